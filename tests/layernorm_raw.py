"""Raw C-ABI harness for csts_amd/csrc/norm.hip -- csts_layernorm_fwd / _fwd_add / _bwd / _bwd_ex / _bwd2, csts_reduce_rows /
_batched / _wide -- against the fp64 reference and the bars of tests/layernorm_reference.py.  Shared by tests/test_gpu_layernorm.py
(bf16 library) and tests/layernorm_worker.py (a child process on the fp16 library); not a test module itself.

Every tensor of a call is a Buf: n elements inside a wider flat buffer, GUARD elements in front and behind, optionally `mis`
elements further in, which breaks the 16-byte alignment the W = 8 forms of the kernels need and so reaches the W = 1 forms at C % 8 == 0.
  inputs : the whole buffer is NaN except the operand itself: a kernel that reads outside it ends with a non-finite output (lanes
           and rows past the end read CLAMPED addresses of the operand itself).
  outputs: the operand is pre-filled with one NaN bit pattern, everything else with another (the sentinel).  After the call every
           owned element must be finite and every guard element still the sentinel, bit for bit; the buffer of an output the call
           was told not to write (NULL statistics, a deferred dgamma | dbeta) still holds its pre-fill.
Each runner returns one plain dict per checked tensor group: flags (finite, guards, *_equal), derived ratios |err| / bar (mean_ratio,
copy_ratio, ratio: must be <= 1), the constants the measured bars would need (k_y, k_dx, k_dg, k_db: the smallest K with
|err| <= K u S + u_out |ref| at every element; rstd_rel: per row) and min_var, all JSON-serialisable."""
import ctypes as C

import torch

from csts_amd import lib as L
import layernorm_reference as LR

GUARD = 64                                       # elements in front of and behind every operand (keeps 16-byte alignment)
SENT = {4: 0x7FC0DEAD, 2: 0x7FDE}                # the sentinel: a quiet NaN (fp32 / bf16 / fp16) no kernel produces
PREFILL = {4: 0x7FC00001, 2: 0x7FFF}             # what an output holds before the call: another NaN
_IV = {4: torch.int32, 2: torch.int16}
F = torch.float32
LN_BWD_WAVES, LN_BWD_CAP, LN_FWD_CAP = 8, 512, 4096


def _sx(v, es):                                  # the bit pattern as a signed integer of the view's width
    return v - (1 << (8 * es)) if v >= 1 << (8 * es - 1) else v


def stream():
    return torch.cuda.current_stream().cuda_stream


def dt_code(dtype):
    return L.F32 if dtype == F else L.BF16


def tag(dtype):
    return "f32" if dtype == F else "h16"


class Buf:
    """n elements of `dtype` at element GUARD + mis of one flat buffer."""

    def __init__(self, n, dtype, dev, mis=0):
        self.n, self.dtype, self.lo = n, dtype, GUARD + mis
        self.es = torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.empty(2 * GUARD + mis + n, dtype=dtype, device=dev)
        self.ibuf = self.buf.view(_IV[self.es])
        self.ibuf.fill_(_sx(SENT[self.es], self.es))
        assert self.buf.data_ptr() % 16 == 0 and (self.ptr() % 16 == 0) == ((mis * self.es) % 16 == 0)

    def view(self):
        return self.buf[self.lo:self.lo + self.n]

    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.es

    def load(self, data):
        """Input: NaN everywhere (the sentinel), the data in the operand."""
        self.view().copy_(data.reshape(-1).to(self.dtype))
        return self

    def arm(self):
        """Output: the sentinel everywhere, the other NaN in the operand."""
        self.ibuf.fill_(_sx(SENT[self.es], self.es))
        self.ibuf[self.lo:self.lo + self.n].fill_(_sx(PREFILL[self.es], self.es))
        return self

    def guards_ok(self):
        s = _sx(SENT[self.es], self.es)
        return bool((self.ibuf[:self.lo] == s).all()) and bool((self.ibuf[self.lo + self.n:] == s).all())

    def finite(self):
        return bool(torch.isfinite(self.view()).all())

    def untouched(self):
        return self.guards_ok() and bool((self.ibuf[self.lo:self.lo + self.n] == _sx(PREFILL[self.es], self.es)).all())


def _ratio_at(err, bar):
    """Worst |err| / bar and its index; an error where the bar is zero counts as infinite."""
    r = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = r.nan_to_num(nan=float("inf"), posinf=float("inf"))
    i = int(r.argmax())
    idx = []
    for n in reversed(r.shape):
        idx.append(i % n)
        i //= n
    return float(r.max()), list(reversed(idx))


def _ratio(err, bar):
    return _ratio_at(err, bar)[0]


def _k(got, ref, S, dtype):
    """The smallest K with |got - ref| <= K u S + u_out |ref| (+ 2^-25 for fp16 storage) at every element, and where it is needed."""
    excess = ((got - ref).abs() - LR.U_OUT[dtype] * ref.abs() - LR.sub_abs(dtype)).clamp_min(0)
    return _ratio_at(excess, LR.U * S)


OUTPUTS = None                                   # a list (tools/ln_digest.py): every run_* appends (name, output Buf)


def _record(name, **bufs):
    if OUTPUTS is not None:
        OUTPUTS.extend((f"{name} | {k}", b) for k, b in bufs.items() if b is not None)


def _mis(mis, name):
    return mis[1] if mis is not None and mis[0] == name else 0


# The launch geometry of norm.hip, mirrored so that a test can state how many trips of a grid-stride loop its rows take.
def group_lanes(C):
    return 16 if C <= 128 else (32 if C <= 256 else 64)


def rows_per_wave(C):
    return 4 if C <= 192 else (2 if C <= 384 else 1)


def fwd_grid(rows, C, vec):
    """(workgroups, uncapped workgroups, rows one pass of the whole grid covers) of a forward launch."""
    per = (256 // group_lanes(C)) * 2 if vec else 4 * rows_per_wave(C)
    want = -(-rows // per)
    return min(want, LN_FWD_CAP), want, min(want, LN_FWD_CAP) * per


def bwd_grid(rows, C, vec):
    """The same for a backward launch (one segment).  The W = 8 form takes one row per lane group and pass."""
    want = -(-rows // (LN_BWD_WAVES * rows_per_wave(C)))
    nb = min(want, LN_BWD_CAP)
    return nb, want, nb * (512 // group_lanes(C) if vec else LN_BWD_WAVES * rows_per_wave(C))


def is_vec(C, mis=None):
    return C % 8 == 0 and mis is None


# ------------------------------------------------------------------------------------------------------------ forward
def run_fwd(rows, C, xdt, ydt, dev, kind="plain", seed=1, eps=1e-6, mis=None, stats=True, add=None, keep=None):
    """csts_layernorm_fwd, or csts_layernorm_fwd_add when `add` names the value set of the addend.  mis = (operand, elements):
    operand in x, y, gamma, beta, addend, sum.  stats False: mean and rstd NULL."""
    lib = L.load()
    n = rows * C
    x = Buf(n, xdt, dev, _mis(mis, "x")).load(LR.values(kind, rows, C, seed, dev))
    g32, b32 = LR.params(C, seed + 1000, dev)
    gamma, beta = Buf(C, F, dev, _mis(mis, "gamma")).load(g32), Buf(C, F, dev, _mis(mis, "beta")).load(b32)
    y = Buf(n, ydt, dev, _mis(mis, "y")).arm()
    mean, rstd = Buf(rows, F, dev).arm(), Buf(rows, F, dev).arm()
    sp = (mean.ptr(), rstd.ptr()) if stats else (None, None)
    if add is None:
        a = s = None
        rc = lib.csts_layernorm_fwd(x.ptr(), dt_code(xdt), gamma.ptr(), beta.ptr(), y.ptr(), dt_code(ydt), sp[0], sp[1], rows, C, eps, stream())
    else:
        a = Buf(n, xdt, dev, _mis(mis, "addend")).load(LR.values(add, rows, C, seed + 50, dev))
        s = Buf(n, xdt, dev, _mis(mis, "sum")).arm()
        rc = lib.csts_layernorm_fwd_add(x.ptr(), a.ptr(), s.ptr(), dt_code(xdt), gamma.ptr(), beta.ptr(), y.ptr(), dt_code(ydt), sp[0], sp[1],
                                        rows, C, eps, stream())
    L.check(rc, "csts_layernorm_fwd")
    torch.cuda.synchronize()
    # With an addend the kernel normalises the sum AS STORED (a 16-bit sum is rounded before the statistics: it is the x the
    # backward reads); sum_equal ties the stored sum to x + addend, so the reference is the LayerNorm of the stored sum.
    x64 = (x if s is None else s).view().double().view(rows, C)
    f = LR.forward(x64, gamma.view().double(), beta.view().double(), eps)
    ky, at = _k(y.view().double().view(rows, C), f["y"], f["S_y"], ydt)
    outs = [y, mean, rstd] + ([s] if s is not None else [])
    r = {"name": f"fwd{'_add' if add else ''} rows {rows} C {C} {tag(xdt)}->{tag(ydt)} {kind}{'' if mis is None else ' mis ' + mis[0] + '+' + str(mis[1])}"
                 f"{'' if stats else ' no stats'}",
         "finite": y.finite() and (s is None or s.finite()), "guards": all(o.guards_ok() for o in outs),
         "k_y": ky, "k_y_at": at, "min_var": float(f["var"].min()),
         "kind": {"rstd_rel": tag(xdt), "k_y": tag(ydt)}}
    if stats:
        r["finite"] = r["finite"] and mean.finite() and rstd.finite()
        r["mean_ratio"] = _ratio((mean.view().double() - f["mean"]).abs(), LR.mean_bar(f["sum"], C))
        r["rstd_rel"] = float(((rstd.view().double() - f["rstd"]).abs() / f["rstd"]).max())
    else:
        r["guards"] = r["guards"] and mean.untouched() and rstd.untouched()
    if s is not None:
        r["sum_equal"] = torch.equal(s.view(), (x.view().float() + a.view().float()).to(xdt))
    if keep is not None:
        keep.update(y=y.view().clone(), mean=mean.view().clone(), rstd=rstd.view().clone(), sum=None if s is None else s.view().clone(),
                    gamma=g32, ref=f)
    _record(r["name"], y=y, mean=mean, rstd=rstd, sum_out=s)
    return [r]


# ------------------------------------------------------------------------------------------------------------ backward
class _BwdProblem:
    """Operands of one LayerNorm backward over `segs` stacked tensors of (rows, C) and the fp64 reference of each segment.  mean and
    rstd are the fp64 statistics of the x the kernel reads, rounded to fp32: what a forward stores."""

    def __init__(self, rows, C, dydt, xdt, dev, kinds, seed, eps, mis=None, dy2=False, addend=False, x_data=None, stats=None):
        self.rows, self.C, self.segs, n = rows, C, len(kinds), rows * C
        xs = [LR.values(k, rows, C, seed + 10 * i, dev) for i, k in enumerate(kinds)] if x_data is None else [x_data]
        self.x = Buf(n * self.segs, xdt, dev, _mis(mis, "x")).load(torch.cat(xs))
        self.dy = Buf(n * self.segs, dydt, dev, _mis(mis, "dy")).load(torch.cat([LR.values("plain", rows, C, seed + 100 + 10 * i, dev) for i in range(self.segs)]))
        self.dy2 = Buf(n, dydt, dev, _mis(mis, "dy2")).load(LR.values("plain", rows, C, seed + 200, dev)) if dy2 else None
        self.addend = Buf(n, xdt, dev, _mis(mis, "addend")).load(LR.values("plain", rows, C, seed + 300, dev)) if addend else None
        self.gammas = [Buf(C, F, dev, _mis(mis, "gamma")).load(LR.params(C, seed + 1000 + i, dev)[0]) for i in range(self.segs)]
        self.mean, self.rstd = Buf(rows * self.segs, F, dev), Buf(rows * self.segs, F, dev)
        self.dx = Buf(n * self.segs, xdt, dev, _mis(mis, "dx")).arm()
        self.ref, self.min_var = [], []
        for i in range(self.segs):
            x64 = self.x.view()[i * n:(i + 1) * n].double().view(rows, C)
            f = LR.forward(x64, self.gammas[i].view().double(), torch.zeros(C, dtype=torch.float64, device=dev), eps)
            self.mean.view()[i * rows:(i + 1) * rows] = f["mean"].float()
            self.rstd.view()[i * rows:(i + 1) * rows] = f["rstd"].float()
            self.min_var.append(float(f["var"].min()))
        for i in range(self.segs):
            sl = slice(i * n, (i + 1) * n)
            self.ref.append(LR.backward(self.dy.view()[sl].double().view(rows, C), self.x.view()[sl].double().view(rows, C),
                                        self.gammas[i].view().double(), self.mean.view()[i * rows:(i + 1) * rows].double(),
                                        self.rstd.view()[i * rows:(i + 1) * rows].double(),
                                        dy2=None if self.dy2 is None else self.dy2.view().double().view(rows, C),
                                        addend=None if self.addend is None else self.addend.view().double().view(rows, C)))
        if stats is not None:                     # the kernel reads a forward kernel's own statistics; the reference keeps those of x
            self.mean.view().copy_(stats[0])
            self.rstd.view().copy_(stats[1])

    def result(self, name, i, dgb, extra_ok=True):
        rows, C, n = self.rows, self.C, self.rows * self.C
        b = self.ref[i]
        kdx, at = _k(self.dx.view()[i * n:(i + 1) * n].double().view(rows, C), b["dx"], b["S_dx"], self.dx.dtype)
        r = {"name": name, "finite": self.dx.finite(), "guards": self.dx.guards_ok() and extra_ok, "min_var": self.min_var[i],
             "k_dx": kdx, "k_dx_at": at,
             "kind": {"k_dx": tag(self.dx.dtype), "k_dg": tag(self.dy.dtype), "k_db": tag(self.dy.dtype)}}
        if dgb is not None:
            r["finite"] = r["finite"] and bool(torch.isfinite(dgb).all())
            r["k_dg"] = _ratio((dgb[:C].double() - b["dgamma"]).abs(), LR.U * b["S_dg"])
            r["k_db"] = _ratio((dgb[C:].double() - b["dbeta"]).abs(), LR.U * b["S_db"])
        return r


def bwd_partial_rows(rows, C):
    """Partial rows of 2 C floats a backward launch writes per segment: csts_layernorm_bwd_workspace(rows, C) / (2 C 4)."""
    wsz = L.load().csts_layernorm_bwd_workspace(rows, C)
    assert wsz > 0 and wsz % (2 * C * 4) == 0
    return wsz // (2 * C * 4)


def run_bwd(rows, C, dydt, xdt, dev, kind="plain", seed=2, eps=1e-6, mis=None, dy2=False, addend=False, copy=None, deferred=False,
            keep=None, x_data=None, stats=None, ex=False):
    """csts_layernorm_bwd (csts_layernorm_bwd_ex with dy2, a copy scale or ex=True).  copy: None | "plain" (the 16-bit copy of dx) |
    rows_per_scale (the copy times scale[row / rps]; one scale is 0 when there are several).  deferred: dgamma / dbeta NULL, the
    partial rows of the workspace finished here with csts_reduce_rows.  x_data: the x to use instead of a value set; stats: the
    (mean, rstd) the kernel is handed instead of the fp64 statistics of that x (the reference keeps the latter)."""
    lib = L.load()
    H = L.half_dtype()
    p = _BwdProblem(rows, C, dydt, xdt, dev, (kind,), seed, eps, mis, dy2, addend, x_data, stats)
    nb = bwd_partial_rows(rows, C)
    ws, dgb = Buf(nb * 2 * C, F, dev).arm(), Buf(2 * C, F, dev).arm()
    c16 = Buf(rows * C, H, dev, _mis(mis, "copy")).arm() if copy is not None else None
    scale = rps = None
    if copy is not None and copy != "plain":
        rps = int(copy)
        assert rows % rps == 0 and xdt == F, "the bar of the scaled copy is stated against an fp32 dx"
        sc = 0.5 + torch.rand(rows // rps, generator=torch.Generator().manual_seed(seed + 400))
        if sc.numel() > 1:
            sc[sc.numel() // 2] = 0.0
        scale = Buf(rows // rps, F, dev).load(sc.to(dev))
    dg_ptr, db_ptr = (None, None) if deferred else (dgb.ptr(), dgb.ptr() + 4 * C)
    cp = None if c16 is None else c16.ptr()
    if dy2 or scale is not None or ex:
        rc = lib.csts_layernorm_bwd_ex(p.dy.ptr(), None if p.dy2 is None else p.dy2.ptr(), dt_code(dydt), p.x.ptr(), dt_code(xdt), p.gammas[0].ptr(),
                                       p.mean.ptr(), p.rstd.ptr(), p.dx.ptr(), dt_code(xdt), None if p.addend is None else p.addend.ptr(), cp,
                                       None if scale is None else scale.ptr(), rps or 1, dg_ptr, db_ptr, ws.ptr(), nb * 2 * C * 4, rows, C, stream())
    else:
        rc = lib.csts_layernorm_bwd(p.dy.ptr(), dt_code(dydt), p.x.ptr(), dt_code(xdt), p.gammas[0].ptr(), p.mean.ptr(), p.rstd.ptr(), p.dx.ptr(),
                                    dt_code(xdt), None if p.addend is None else p.addend.ptr(), cp, dg_ptr, db_ptr, ws.ptr(), nb * 2 * C * 4, rows, C, stream())
    L.check(rc, "csts_layernorm_bwd")
    torch.cuda.synchronize()
    ok = ws.finite() and ws.guards_ok() and dgb.guards_ok()
    if deferred:                                  # nothing but the partial rows was written; the caller's second stage
        ok = ok and dgb.untouched()
        L.check(lib.csts_reduce_rows(ws.ptr(), dgb.ptr(), nb, 2 * C, 1.0, stream()), "csts_reduce_rows")
        torch.cuda.synchronize()
        ok = ok and dgb.guards_ok()
    name = (f"bwd rows {rows} C {C} dy {tag(dydt)} x {tag(xdt)} {kind}{'' if mis is None else ' mis ' + mis[0] + '+' + str(mis[1])}"
            f"{' dy2' if dy2 else ''}{' addend' if addend else ''}{'' if copy is None else ' copy ' + str(copy)}{' deferred' if deferred else ''}")
    r = p.result(name, 0, dgb.view(), ok)
    if c16 is not None:
        r["finite"] = r["finite"] and c16.finite()
        r["guards"] = r["guards"] and c16.guards_ok()
        if xdt == F:
            stored = p.dx.view().double().view(rows, C)
            s64 = None if scale is None else scale.view().double()
            want = stored if s64 is None else stored * LR.row_scale(s64, rows, rps)
            r["copy_ratio"] = _ratio((c16.view().double().view(rows, C) - want).abs(), LR.copy_bar(stored, s64, rps, H))
            if s64 is not None and s64.numel() > 1:
                z = s64.numel() // 2
                r["copy_zero_equal"] = bool((c16.view().view(rows, C)[z * rps:(z + 1) * rps] == 0).all())
        else:                                     # a 16-bit dx and its unscaled copy are the same rounding of the same fp32 value
            r["copy_equal"] = torch.equal(c16.view(), p.dx.view())
    if keep is not None:
        keep.update(dx=p.dx.view().clone(), dgb=dgb.view().clone(), ws=ws.view().clone(), copy=None if c16 is None else c16.view().clone())
    _record(name, dx=p.dx, copy16=c16, ws=ws, dgb=dgb)
    return [r]


def run_bwd2(rows, C, dydt, xdt, dev, kinds=("plain", "offset"), seed=3, eps=1e-5):
    """csts_layernorm_bwd2: two stacked tensors with gamma0 != gamma1 and one value set each; dgb0 / dgb1 against the reference of
    their own segment.  Then segment 0 alone through csts_layernorm_bwd at the same rows: the same grid, the same kernel
    (blockIdx.y == 0 adds no offset anywhere) and the same second stage, so dx, the partial rows and dgamma | dbeta are the same
    bits by construction (seg0_equal)."""
    lib = L.load()
    p = _BwdProblem(rows, C, dydt, xdt, dev, kinds, seed, eps)
    n, nb = rows * C, bwd_partial_rows(rows, C)
    ws = Buf(2 * nb * 2 * C, F, dev).arm()
    dgbs = [Buf(2 * C, F, dev).arm(), Buf(2 * C, F, dev).arm()]
    L.check(lib.csts_layernorm_bwd2(p.dy.ptr(), dt_code(dydt), p.x.ptr(), dt_code(xdt), p.gammas[0].ptr(), p.gammas[1].ptr(), p.mean.ptr(),
                                    p.rstd.ptr(), p.dx.ptr(), dt_code(xdt), dgbs[0].ptr(), dgbs[1].ptr(), ws.ptr(), 2 * nb * 2 * C * 4, rows, C,
                                    stream()), "csts_layernorm_bwd2")
    torch.cuda.synchronize()
    ok = ws.finite() and ws.guards_ok() and dgbs[0].guards_ok() and dgbs[1].guards_ok()
    res = [p.result(f"bwd2[{i}] rows {rows} C {C} dy {tag(dydt)} x {tag(xdt)} {kinds[i]}", i, dgbs[i].view(), ok) for i in range(2)]
    _record(f"bwd2 rows {rows} C {C} dy {tag(dydt)} x {tag(xdt)}", dx=p.dx, ws=ws, dgb0=dgbs[0], dgb1=dgbs[1])
    one = {}
    run_bwd(rows, C, dydt, xdt, dev, kind=kinds[0], seed=seed, eps=eps, keep=one)
    res[0]["seg0_equal"] = (torch.equal(one["dx"], p.dx.view()[:n]) and torch.equal(one["dgb"], dgbs[0].view())
                            and torch.equal(one["ws"], ws.view()[:nb * 2 * C]))
    return res


# ------------------------------------------------------------------------------------------------------------ reducers
def run_reduce(nrows, ncols, scale, dev, seed=5):
    """csts_reduce_rows: bit-equal to the exact-order emulation of reduce_rows_kernel<RL>, inside the derived bar against fp64,
    the same bits from a second call."""
    lib = L.load()
    ws = Buf(nrows * ncols, F, dev).load(LR.mixed(nrows, ncols, seed + nrows + ncols, dev))
    outs = [Buf(ncols, F, dev).arm(), Buf(ncols, F, dev).arm()]
    for o in outs:
        L.check(lib.csts_reduce_rows(ws.ptr(), o.ptr(), nrows, ncols, scale, stream()), "csts_reduce_rows")
    torch.cuda.synchronize()
    w = ws.view().view(nrows, ncols)
    RL = LR.reduce_rl(nrows)
    ref, absum = LR.reduce_ref(w, scale)
    return [{"name": f"reduce_rows<{RL}> {nrows} x {ncols} scale {scale}", "finite": outs[0].finite(), "guards": all(o.guards_ok() for o in outs),
             "emulation_equal": torch.equal(outs[0].view(), LR.reduce_rows_emulation(w, scale, RL)),
             "repeat_equal": torch.equal(outs[0].view(), outs[1].view()),
             "ratio": _ratio((outs[0].view().double() - ref).abs(), LR.reduce_bar(absum, scale, nrows, RL))}]


def run_reduce_table(items, max_ncols, dev, wide=False, seed=6):
    """csts_reduce_rows_batched / csts_reduce_rows_wide: items = [(nrows, ncols, scale)] in ONE launch, the descriptor table built
    with L.ReduceDesc and uploaded as ops.py does.  Batched: bit-equal to the RL = 32 emulation, and to csts_reduce_rows on the same
    data where that runs reduce_rows_kernel<32> too (nrows > 64).  Wide: bit-equal to the sequential emulation."""
    lib = L.load()
    wss = [Buf(nr * nc, F, dev).load(LR.mixed(nr, nc, seed + i, dev)) for i, (nr, nc, _) in enumerate(items)]
    outs = [Buf(nc, F, dev).arm() for _, nc, _ in items]
    descs = (L.ReduceDesc * len(items))()
    for i, (nr, nc, sc) in enumerate(items):
        assert not wide or (nc % 4 == 0 and wss[i].ptr() % 16 == 0 and outs[i].ptr() % 16 == 0)
        descs[i].ws, descs[i].out, descs[i].nrows, descs[i].ncols, descs[i].scale = wss[i].ptr(), outs[i].ptr(), nr, nc, sc
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    fn = lib.csts_reduce_rows_wide if wide else lib.csts_reduce_rows_batched
    L.check(fn(table.data_ptr(), len(items), max_ncols, stream()), "csts_reduce_rows_batched / _wide")
    torch.cuda.synchronize()
    res = []
    for i, (nr, nc, sc) in enumerate(items):
        w = wss[i].view().view(nr, nc)
        ref, absum = LR.reduce_ref(w, sc)
        emu = LR.reduce_wide_emulation(w, sc) if wide else LR.reduce_rows_emulation(w, sc, 32)
        r = {"name": f"reduce_{'wide' if wide else 'batched'}[{i}] {nr} x {nc} scale {sc}", "finite": outs[i].finite(), "guards": outs[i].guards_ok(),
             "emulation_equal": torch.equal(outs[i].view(), emu),
             "ratio": _ratio((outs[i].view().double() - ref).abs(), LR.reduce_bar(absum, sc, nr, None if wide else 32))}
        if not wide and nr > 64:
            single = Buf(nc, F, dev).arm()
            L.check(lib.csts_reduce_rows(wss[i].ptr(), single.ptr(), nr, nc, sc, stream()), "csts_reduce_rows")
            torch.cuda.synchronize()
            r["single_equal"] = torch.equal(outs[i].view(), single.view())
        res.append(r)
    return res


# ------------------------------------------------------------------------------------------------------------ verdicts
DERIVED = ("mean_ratio", "copy_ratio", "ratio")
MEASURED = ("rstd_rel", "k_y", "k_dx", "k_dg", "k_db")


def worst(results, key):
    return max((r[key] for r in results if key in r), default=0.0)


def bar_of(bars, r, key, half):
    """bars = {key: {"f32" | "bf16" | "fp16": bound}}: the bound for the storage kind of the tensor the key measures."""
    return bars[key]["f32" if r["kind"][key] == "f32" else half]


def violations(results, bars, half="bf16"):
    """Every result that wrote a non-finite element, touched a guard, misses a bit-equality, a derived bar (ratio <= 1) or one of
    the measured bars; every measured key a result carries must have a bound."""
    bad = []
    for r in results:
        ok = r["finite"] and r["guards"] and all(v is True for k, v in r.items() if k.endswith("_equal"))
        ok = ok and all(r[k] <= 1.0 for k in DERIVED if k in r) and all(r[k] <= bar_of(bars, r, k, half) for k in MEASURED if k in r)
        if not ok:
            bad.append(r)
    return bad


# ----------------------------------------------------------------------------------------------- shared problem sets
VEC_C = (8, 16, 24, 40, 96, 128, 136, 192, 256, 264, 384, 512, 520, 768)
SCALAR_C = (1, 7, 63, 65, 100, 129, 191, 250, 383, 500, 767)
SMALL_ROWS = (1, 3, 5, 33, 77, 257)
KINDS = ("plain", "offset")


def small_table(C, pairs):
    """The small-instantiation runs of one C as (rows, dtype pair, value set): every rows of SMALL_ROWS once, with the dtype pairs and
    the value sets dealt round-robin (six rows: every pair and both sets at every C), then every pair on both sets at rows = 33 -- a
    ragged last pass of the forward W = 8 forms (2 rows per group) and of the W = 1 forms (4 / 2 rows per wave), and more rows
    than one pass of the backward W = 8 forms covers at C 136 to 192 and 264 to 384 (a second trip of some lane groups)."""
    ci = (VEC_C + SCALAR_C).index(C)
    t = [(rows, pairs[(i + ci) % len(pairs)], KINDS[i % 2]) for i, rows in enumerate(SMALL_ROWS)]
    return t + [(33, pr, k) for pr in pairs for k in KINDS]


def small_fwd(C, dev, pairs, eps=1e-6):
    res = []
    for rows, (xdt, ydt), kind in small_table(C, pairs):
        res += run_fwd(rows, C, xdt, ydt, dev, kind=kind, seed=rows + C, eps=eps)
    xdt, ydt = pairs[C % len(pairs)]
    return res + run_fwd(5, C, xdt, ydt, dev, kind="offset", seed=C, eps=eps, stats=False)


def small_bwd(C, dev, pairs, eps=1e-6):
    res = []
    for rows, (dydt, xdt), kind in small_table(C, pairs):
        res += run_bwd(rows, C, dydt, xdt, dev, kind=kind, seed=rows + C, eps=eps)
    return res


def fwd_add_cases(dev, H):
    """csts_layernorm_fwd_add: fp32 and 16-bit x, W = 8 and W = 1 widths, odd rows (a ragged last pass of every form)."""
    res = []
    for C in (8, 96, 100, 191, 384, 768):
        for xdt, ydt in ((F, F), (F, H), (H, H), (H, F)):
            res += run_fwd(77 if C < 384 else 33, C, xdt, ydt, dev, kind="offset", seed=C, add="plain", eps=1e-6)
    return res


def bwd_ex_cases(dev, H, C):
    """csts_layernorm_bwd_ex at one C, rows = 70: dy2 / addend present or absent, the 16-bit copy without a scale and with
    rows_per_scale 7, 70 and rows (one scale of 0 among several), with 16-bit dy and 16-bit x."""
    res = []
    for dy2 in (False, True):
        for addend in (False, True):
            res += run_bwd(70, C, F, F, dev, kind="offset", seed=C, dy2=dy2, addend=addend, ex=True)
            res += run_bwd(70, C, H, H, dev, kind="plain", seed=C + 1, dy2=dy2, addend=addend, copy="plain", ex=True)
    for copy in ("plain", 7, 70):
        res += run_bwd(70, C, F, F, dev, kind="plain", seed=C + 2, copy=copy, dy2=True, addend=True)
        res += run_bwd(70, C, H, F, dev, kind="offset", seed=C + 3, copy=copy)
    return res + run_bwd(140, C, F, F, dev, kind="plain", seed=C + 4, copy=70)


def misaligned_cases(dev, H, C):
    """One operand at a time off its 16-byte alignment (fp32: one element; 16-bit: one and three) at a width the W = 8 forms would
    otherwise take."""
    res = []
    for op in ("x", "y", "gamma", "beta"):
        res += run_fwd(33, C, F, F, dev, kind="offset", seed=C, mis=(op, 1))
    for op, k in (("x", 1), ("x", 3), ("y", 1), ("y", 3)):
        res += run_fwd(33, C, H, H, dev, kind="offset", seed=C + 1, mis=(op, k))
    for op in ("addend", "sum"):
        res += run_fwd(33, C, F, H, dev, kind="offset", seed=C + 2, mis=(op, 1), add="plain")
        res += run_fwd(33, C, H, F, dev, kind="plain", seed=C + 3, mis=(op, 3), add="plain")
    for op in ("dy", "x", "dx", "gamma", "addend", "copy"):
        res += run_bwd(33, C, F, F, dev, kind="offset", seed=C + 4, mis=(op, 1), addend=True, copy="plain")
    for op, k in (("dy", 1), ("dy", 3), ("x", 3), ("dx", 1), ("addend", 3), ("dy2", 1)):
        res += run_bwd(33, C, H, H, dev, kind="offset", seed=C + 5, mis=(op, k), addend=True, dy2=True)
    return res


MISALIGNED_C = (96, 192, 384, 768)


def fwd_trips(H):
    """Grid-stride trips of a forward launch: (C, rows, x dtype, y dtype), rows just past the 4096-workgroup cap."""
    return [(96, 131072 + 35, H, H), (768, 32768 + 9, F, H), (100, 65536 + 7, F, F)]


def bwd_trips(H):
    """The same for a backward launch: (C, rows, dy dtype, x dtype, whether the grid is capped at 512)."""
    return [(96, 16384 + 37, F, F, True), (192, 8192 + 19, H, F, False), (192, 16384 + 19, F, H, True), (384, 4096 + 9, H, H, False),
            (384, 8192 + 9, F, F, True), (768, 4096 + 9, H, F, True), (100, 16384 + 5, F, F, True), (383, 8192 + 3, H, H, True),
            (767, 4096 + 3, F, H, True)]


DEFERRED = [(96, 77), (100, 300), (192, 2100), (768, 4096 + 9)]         # (C, rows): 3, 10, 66 and 512 partial rows
BWD2 = [(C, rows) for C in (8, 96, 192) for rows in (5, 77, 16384 + 37)] + [(7, 5), (100, 77), (191, 16384 + 37)]


def bwd2_pairs(C, rows, H):
    """The (dy, x) dtype pairs test_bwd2 runs at (C, rows)."""
    return ((F, F), (H, H)) if rows < 1000 else (((H, F),) if C != 96 else ((F, H),))
