"""Raw C-ABI harness for csts_gemm (csts_amd/csrc/gemm.hip, gemm4.hip, gemm5.hip) through L.GemmArgs, against the fp64 reference
and the bars of tests/gemm_reference.py, and the case tables.  Shared by tests/test_gpu_gemm.py (bf16 library),
tests/gemm_worker.py (child processes: the fp16 library, the switch-reached kernels) and tests/test_gemm_reference_host.py (names
and references only: nothing here touches a GPU until run() is called); not a test module itself.

Every operand is a Win: rows x cols inside a wider flat buffer, GUARD elements in front and behind, leading dimension cols + pad,
optionally `mis` elements further in (which breaks the 16-byte alignment the vector kernels need).
  inputs : the whole buffer is NaN (the sentinel) except the rows x cols themselves, pad columns included: a kernel that multiplies
           anything outside its operand ends with a non-finite output.
  outputs: C, aux, colsum and the split-K workspace are pre-filled with one NaN pattern and surrounded, pad columns included, by
           another (the sentinel).  After a call every owned element is finite, every sentinel intact bit for bit, and an output
           the call was told not to write (aux under DGELU is an input; the workspace beyond nsplit slabs) still holds its pre-fill.
           With atomic split-K C is pre-zeroed instead, as the library asks.
run() returns one plain JSON-serialisable dict: flags (finite, guards, c_equal, aux_equal, ws_tail, colsum_*), the name of the kernel
csts_gemm_kernel_name gives for the REAL arguments, k / k_aux (the smallest constant with |err| <= k u S + u_out |ref| at every
element, and where) for cases without an activation, cf (the c_f the function term needs, given k) for GELU / DGELU,
c_derived, and colsum_ratio = |err| / (2 (K + nsplit) u colsum|A|), which must be <= 1."""
import ctypes as C
import itertools

import torch

from csts_amd import lib as L
import gemm_reference as GR

GUARD = 256                                      # elements in front of and behind every operand (keeps 16-byte alignment)
SENT = {4: 0x7FC0DEAD, 2: 0x7FDE}                # the sentinel: a quiet NaN (fp32 / bf16 / fp16) no kernel produces
PREFILL = {4: 0x7FC00001, 2: 0x7FFF}             # what an output holds before the call: another NaN
_IV = {4: torch.int32, 2: torch.int16}
F = torch.float32
LAYOUT = {"NT": L.GEMM_NT, "NN": L.GEMM_NN, "TN": L.GEMM_TN}
EPI = {"none": L.EPI_NONE, "gelu": L.EPI_GELU, "dgelu": L.EPI_DGELU}
OPERANDS = ("A", "B", "C", "bias", "aux", "residual", "row_scale", "workspace", "colsum")
FAKE = {n: (i + 1) << 32 for i, n in enumerate(OPERANDS)}      # made-up 256-byte-aligned addresses for the host-only name query


def _sx(v, es):
    return v - (1 << (8 * es)) if v >= 1 << (8 * es - 1) else v


def stream():
    return torch.cuda.current_stream().cuda_stream


def code(name):
    return L.F32 if name == "f32" else L.BF16


def kind_of(dtype):
    return "f32" if dtype == F else L.HALF


class Win:
    """rows x cols of `dtype`, leading dimension cols + pad, at element GUARD + mis of one flat buffer."""

    def __init__(self, rows, cols, dtype, dev, pad=0, mis=0):
        self.rows, self.cols, self.ld, self.dtype, self.lo = rows, cols, cols + pad, dtype, GUARD + mis
        self.es = torch.empty(0, dtype=dtype).element_size()
        self.n = rows * self.ld
        self.buf = torch.empty(2 * GUARD + mis + self.n, dtype=dtype, device=dev)
        self.ibuf = self.buf.view(_IV[self.es])
        self.ibuf.fill_(_sx(SENT[self.es], self.es))
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.es

    def _own(self, t):
        return t[self.lo:self.lo + self.n].view(self.rows, self.ld)[:, :self.cols]

    def view(self):
        return self._own(self.buf)

    def load(self, data):
        self.view().copy_(data.reshape(self.rows, self.cols).to(self.dtype))
        return self

    def arm(self, zero=False):
        self.ibuf.fill_(_sx(SENT[self.es], self.es))
        self._own(self.ibuf).fill_(0 if zero else _sx(PREFILL[self.es], self.es))
        return self

    def guards_ok(self):
        t = self.ibuf.clone()
        self._own(t).fill_(_sx(SENT[self.es], self.es))
        return bool((t == _sx(SENT[self.es], self.es)).all())

    def finite(self):
        return bool(torch.isfinite(self.view()).all())

    def prefilled(self, lo=0):
        """Columns lo .. of the (single-row) window still hold the pre-fill."""
        return bool((self._own(self.ibuf)[:, lo:] == _sx(PREFILL[self.es], self.es)).all())


def _worst(err, bar):
    """Worst |err| / bar and its index; an error where the bar is zero counts as infinite."""
    r = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = r.nan_to_num(nan=float("inf"), posinf=float("inf"))
    i = int(r.argmax())
    return float(r.flatten()[i]), [i // r.shape[-1], i % r.shape[-1]] if r.dim() == 2 else [i]


# ------------------------------------------------------------------------------------------------------------ arguments
def shapes(c):
    """(rows, cols) of A, B as stored."""
    return ((c["K"], c["M"]) if c["layout"] == "TN" else (c["M"], c["K"]),
            (c["N"], c["K"]) if c["layout"] == "NT" else (c["K"], c["N"]))


def res_rows(c):
    if c["res_up"]:
        Ti, Hi, Wi, To, Ho, Wo = c["res_up"]
        return c["M"] // (To * Ho * Wo) * Ti * Hi * Wi
    return c["res_row_mod"] if c["res_row_mod"] > 0 else c["M"]


def ws_bytes(c):
    return int(L.load().csts_gemm_splitk_workspace(c["M"], c["N"], c["K"], c["split"])) if c["split"] > 1 and c["det"] else 0


def build_args(c, ptrs):
    """csts_gemm_args of a case; ptrs: operand name -> address (the FAKE ones, plus the case's misalignments, for a name query)."""
    (ar, ac), (br, bc) = shapes(c)
    pad = c["pad"]
    g = L.GemmArgs()
    g.layout = LAYOUT[c["layout"]]
    g.M, g.N, g.K = c["M"], c["N"], c["K"]
    g.A, g.a_dt, g.lda = ptrs["A"], code(c["a"]), ac + pad
    g.B, g.b_dt, g.ldb = ptrs["B"], code(c["b"]), bc + pad
    g.C, g.c_dt, g.ldc = ptrs["C"], code(c["c"]), c["N"] + pad
    g.bias = ptrs["bias"] if c["bias"] else None
    g.epilogue = EPI[c["epi"]]
    if c["aux"] is not None:
        g.aux, g.aux_dt, g.ldaux = ptrs["aux"], code(c["aux"]), c["N"] + pad
    elif c["epi"] == "gelu":
        g.aux_dt = code(c["gelu_dt"])
    if c["res"] is not None:
        g.residual, g.r_dt, g.ldr, g.res_row_mod = ptrs["residual"], code(c["res"]), c["N"] + pad, c["res_row_mod"]
    if c["rps"] > 0:
        g.row_scale, g.rows_per_scale = ptrs["row_scale"], c["rps"]
    g.compute, g.split_k, g.tile_rows, g.algo = code(c["compute"]), c["split"], c["tile_rows"], c["algo"]
    if c["split"] > 1 and c["det"]:
        g.workspace, g.ws_bytes = ptrs["workspace"], ws_bytes(c)
    if c["colsum"]:
        g.colsum = ptrs["colsum"]
    for i, v in enumerate(c["res_up"] or ()):
        g.res_up[i] = v
    return g


def kernel_name(g):
    lib = L.load()
    buf, ns = C.create_string_buffer(160), C.c_int(0)
    rc = lib.csts_gemm_kernel_name(C.byref(g), buf, 160, C.byref(ns))
    return (buf.value.decode() if rc == 0 else "rc -1 " + (lib.csts_last_error() or b"").decode()), ns.value


def host_name(c):
    """(kernel name, k-splits) for made-up pointers with the case's alignment (host-only: nothing is dereferenced)."""
    es = {"A": c["a"], "B": c["b"], "C": c["c"], "aux": c["aux"] or "f32", "residual": c["res"] or "f32"}
    mis = c["mis"] or {}
    ptrs = {n: FAKE[n] + mis.get(n, 0) * (4 if es.get(n, "f32") == "f32" else 2) for n in OPERANDS}
    return kernel_name(build_args(c, ptrs))


# ------------------------------------------------------------------------------------------------------------ one call
def run(c, dev, bars, keep=None, twice=False):
    """One csts_gemm call of case c on device dev, checked against the fp64 reference.  bars: the BARS table of
    tests/test_gpu_gemm.py (cf of a GELU / DGELU case is what the function term needs once k is min(c_derived, bars k)).
    keep: a dict that receives the C the kernel wrote (and the workspace slabs).  twice: call again and compare the bits."""
    lib, half = L.load(), L.half_dtype()
    M, N, pad = c["M"], c["N"], c["pad"]
    mis = c["mis"] or {}
    o = GR.operands(c, half, dev)
    (ar, ac), (br, bc) = shapes(c)
    w = {"A": Win(ar, ac, GR.dt(c["a"], half), dev, pad, mis.get("A", 0)).load(o["A"]),
         "B": Win(br, bc, GR.dt(c["b"], half), dev, pad, mis.get("B", 0)).load(o["B"]),
         "C": Win(M, N, GR.dt(c["c"], half), dev, pad, mis.get("C", 0)).arm(zero=c["zero_c"])}
    if c["bias"]:
        w["bias"] = Win(1, N, F, dev).load(o["bias"])
    if c["aux"] is not None:
        w["aux"] = Win(M, N, GR.dt(c["aux"], half), dev, pad, mis.get("aux", 0))
        w["aux"] = w["aux"].load(o["aux_in"]) if c["epi"] == "dgelu" else w["aux"].arm()
    if c["res"] is not None:
        w["residual"] = Win(res_rows(c), N, GR.dt(c["res"], half), dev, pad, mis.get("residual", 0)).load(o["residual"])
    if c["rps"] > 0:
        w["row_scale"] = Win(1, GR.cdiv(M, c["rps"]), F, dev).load(o["row_scale"])
    nws = ws_bytes(c) // 4
    if nws:
        w["workspace"] = Win(1, nws, F, dev).arm()
    if c["colsum"]:
        w["colsum"] = Win(1, M, F, dev).arm()
    g = build_args(c, {n: (w[n].ptr() if n in w else 0) for n in OPERANDS})
    name, nsplit = kernel_name(g)
    plan = GR.split_plan(c, name) if c["split"] > 1 else (c["K"], 1)
    fn = GR.fn_kind(c, name)
    ref = GR.reference(c, o, half, fn, plan)
    L.check(lib.csts_gemm(C.byref(g), stream()), "csts_gemm " + name)
    torch.cuda.synchronize()
    cdt = w["C"].dtype
    got = w["C"].view().clone()
    fam = name.split("_kernel")[0]
    res = {"kernel": name, "nsplit": nsplit, "plan_nsplit": plan[1], "family": fam, "storage": kind_of(cdt), "fn": fn, "epi": c["epi"],
           "c_derived": ref["c_derived"], "finite": w["C"].finite(), "guards": all(x.guards_ok() for x in w.values()),
           "min_S": float(ref["S"].min())}
    if twice:
        w["C"].arm(zero=c["zero_c"])
        L.check(lib.csts_gemm(C.byref(g), stream()), "csts_gemm " + name)
        torch.cuda.synchronize()
        res["twice_equal"] = bool(torch.equal(w["C"].view().view(_IV[w["C"].es]), got.view(_IV[w["C"].es])))
    err = (got.double() - ref["C64"]).abs()
    excess = (err - GR.U_OUT[cdt] * ref["C64"].abs() - GR.sub_abs(cdt)).clamp_min(0)
    if c["epi"] == "none":
        res["k"], res["k_at"] = _worst(excess, GR.U * ref["S"])
        if c["kind"] == "exact":
            res["c_equal"] = bool(torch.equal(got, ref["C64"].float().to(cdt)))
    else:
        k = min(ref["c_derived"], bars["k"][fam][kind_of(cdt)])
        res["cf"], res["cf_at"] = _worst((excess - k * GR.U * ref["S"] - 2 * GR.U * ref["P"] - ref["fn_base"]).clamp_min(0), GR.U * ref["fn_coef"])
        res["cf_key"] = f"{c['epi']}_{fn}"
    if c["epi"] == "gelu" and c["aux"] is not None:
        adt = w["aux"].dtype
        a = w["aux"].view()
        res["aux_finite"] = w["aux"].finite()
        ex = ((a.double() - ref["pre64"]).abs() - GR.U_OUT[adt] * ref["pre64"].abs() - GR.sub_abs(adt)).clamp_min(0)
        res["k_aux"], res["k_aux_at"] = _worst(ex, GR.U * ref["S_pre"])
        res["aux_storage"] = kind_of(adt)
        if c["kind"] == "exact":
            res["aux_equal"] = bool(torch.equal(a, ref["pre64"].float().to(adt)))
    if c["epi"] == "dgelu":                      # aux is an input there: the call must leave it as it was
        res["aux_kept"] = bool(torch.equal(w["aux"].view(), o["aux_in"]))
    if nws:
        used = nsplit * M * (N + (1 if c["colsum"] else 0))
        res["ws_finite"] = bool(torch.isfinite(w["workspace"].view()[:, :used]).all())
        res["ws_tail"] = w["workspace"].prefilled(used)
        if keep is not None:
            keep["ws"] = w["workspace"].view()[0, :nsplit * M * N].view(nsplit, M, N).clone()
    if c["colsum"]:
        cs = w["colsum"].view()[0].double()
        res["colsum_finite"] = w["colsum"].finite()
        res["colsum_ratio"] = _worst((cs - ref["colsum64"]).abs(), 2 * (c["K"] + nsplit) * GR.U * ref["colsum_abs"])[0]
        if c["kind"] == "exact":
            res["colsum_equal"] = bool(torch.equal(cs, ref["colsum64"]))
    if keep is not None:
        keep["C"], keep["bias"] = got, o["bias"]
    return res


FLAGS = ("finite", "guards", "c_equal", "aux_equal", "aux_finite", "aux_kept", "ws_finite", "ws_tail", "colsum_finite", "colsum_equal",
         "twice_equal")


def misses(r, bars, expect):
    """What of one result does not hold: flags, the kernel name, the bars."""
    bad = [f for f in FLAGS if f in r and r[f] is not True]
    if r["kernel"] != expect:
        bad.append(f"kernel {r['kernel']} != {expect}")
    if r["nsplit"] != r["plan_nsplit"]:
        bad.append("nsplit")
    kb = bars["k"][r["family"]]
    if "k" in r and not r["k"] <= min(r["c_derived"], kb[r["storage"]]):
        bad.append(f"k {r['k']:.3g} at {r['k_at']}")
    if "k_aux" in r and not r["k_aux"] <= min(r["c_derived"], kb[r["aux_storage"]]):
        bad.append(f"k_aux {r['k_aux']:.3g} at {r['k_aux_at']}")
    if "cf" in r and not r["cf"] <= bars["cf"][r["cf_key"]]:
        bad.append(f"cf {r['cf']:.3g} at {r['cf_at']}")
    if "colsum_ratio" in r and not r["colsum_ratio"] <= 1:
        bad.append(f"colsum_ratio {r['colsum_ratio']:.3g}")
    return bad


# ------------------------------------------------------------------------------------------------------------ kernel names
def tf(b):
    return "true" if b else "false"


def name_tiny(layout, wave):
    return f"gemm_tiny_kernel<{LAYOUT[layout]}, {tf(wave)}>"


def name_gemm(layout, f32):
    return f"gemm_kernel<{tf(layout != 'TN')}, {tf(layout == 'NT')}, {tf(f32)}>"


def name_gemm2(layout, a, b, rows):
    return f"gemm2_kernel<{tf(layout != 'TN')}, {tf(layout == 'NT')}, {tf(a == 'f32')}, {tf(b == 'f32')}, {rows // 64}, 2>"


def name_gemm3(mt, s):
    return f"gemm3_kernel<{mt}, {s}>"


# G4_VARIANTS of gemm4.hip: code -> (WM, MT, NT, S, the specialised forms exist, NP)
G4 = {2: (4, 2, 2, 2, False, 0), 3: (4, 2, 2, 3, False, 0), 12: (4, 2, 3, 2, False, 0), 22: (4, 2, 4, 2, False, 0),
      32: (4, 1, 2, 2, True, 0), 33: (4, 1, 2, 3, True, 0), 34: (4, 1, 2, 4, True, 0), 62: (4, 1, 3, 2, True, 0),
      63: (4, 1, 3, 3, True, 0), 64: (4, 1, 3, 4, True, 0), 42: (4, 1, 4, 2, False, 0), 52: (2, 2, 2, 2, False, 0),
      72: (2, 1, 3, 2, True, 0), 73: (2, 1, 3, 3, True, 0), 74: (2, 1, 3, 4, True, 0), 83: (4, 1, 3, 3, True, 4), 84: (4, 1, 2, 3, True, 4)}


def name_gemm4(vcode, form):
    wm, mt, nt, s, _, np_ = G4[vcode]
    return f"gemm4_kernel<{wm}, {mt}, {nt}, {s}, {form}, {np_}>"


def g4_tile(vcode):
    wm, mt, nt, _, _, _ = G4[vcode]
    return wm * 32 * mt, 64 * nt


# launch5 of gemm5.hip: (KCH, NB, W) -> forms
G5 = {(1, 6, 8): (0, 1, 2, 4), (1, 3, 8): (0, 1, 2, 3, 4), (2, 6, 6): (0, 1, 2, 4), (2, 3, 8): (0, 1, 2, 3, 4), (4, 3, 6): (0, 1, 3, 4)}


def name_gemm5(kch, nb, w, form):
    return f"gemm5_kernel<{kch}, {nb}, {w}, {form}>"


def g5_pass_rows(N, nb, w):
    """Rows one pass of the persistent grid of launch5 covers."""
    nt_n = N // (32 * nb)
    return (256 // (8 * nt_n)) * 8 * w * 32


def expected_instantiations():
    """Every instantiation csts_gemm, launch4 and launch5 can start."""
    out = [name_tiny(l, wv) for l in LAYOUT for wv in (False, True)] + [name_gemm(l, f) for l in LAYOUT for f in (False, True)]
    for l, a, b in G2_COMBOS:
        out += [name_gemm2(l, a, b, rows) for rows in (64, 128, 256) if not (rows == 256 and a == "f32")]
    out += [name_gemm3(mt, s) for mt in (1, 2, 4) for s in (2, 3, 4) if not (mt == 4 and s == 4)]
    for v, t in G4.items():
        out += [name_gemm4(v, f) for f in (range(6) if t[4] else (0,))]
    for cfg, forms in G5.items():
        out += [name_gemm5(*cfg, f) for f in forms]
    return sorted(out)


FINISH_FORMS = sorted((v, s) for v in (1, 4) for s in (1, 4, 16))

# ------------------------------------------------------------------------------------------------------------ the cases
# A table is a list of (id, expected kernel name, case); both_kinds() runs every entry once on `exact` values and once on random ones.
case = GR.case
F32C = dict(a="f32", b="f32", c="f32", compute="f32")
RES = dict(c="f32", res="f32")
LAYOUTS = ("NT", "NN", "TN")
G2_COMBOS = [("NT", "h16", "h16"), ("NT", "h16", "f32"), ("NN", "h16", "h16"), ("NN", "h16", "f32"), ("NN", "f32", "h16"),
             ("NN", "f32", "f32"), ("TN", "h16", "h16"), ("TN", "f32", "h16")]
UP = (2, 2, 4, 4, 4, 8)                           # a 2 x 2 x 4 coarse grid under 4 x 4 x 8 fine tokens: 128 rows per batch element


def both_kinds(table):
    out = []
    for i, (cid, name, c) in enumerate(table):
        out.append((f"{cid}-exact", name, dict(c, kind="exact", seed=2 * i + 1)))
        kind = "plain" if i % 2 or c["epi"] == "gelu" else "offset"      # (offset pre-activations are all far up the linear branch of GELU)
        out.append((f"{cid}-{kind}", name, dict(c, kind=kind, seed=2 * i + 2)))
    return out


def tiny_cases():
    """gemm_tiny_kernel: thread mode (K <= 16) and wave mode, three layouts, with and without a bias, odd leading dimensions and A
    off by one element."""
    t = []
    for layout, K, bias in itertools.product(LAYOUTS, (1, 16, 17, 64, 65), (False, True)):
        t.append((f"tiny-{layout}-K{K}-{'bias' if bias else 'plain'}", name_tiny(layout, K > 16),
                  case(layout, 5, 7, K, bias=bias, pad=3, mis={"A": 1}, **F32C)))
    return both_kinds(t)


GENERIC_SHAPES = [(1, 1, 1), (65, 97, 40), (128, 128, 32), (129, 130, 33)]
# every epilogue of gemm_kernel (M = 65 or, for res_up, 256; N = 97; K = 40)
GENERIC_EPIS = [dict(bias=True), dict(bias=True, epi="gelu", aux="f32"), dict(bias=True, epi="gelu", aux="h16", c="h16"), dict(epi="gelu"),
                dict(epi="dgelu", aux="f32"), dict(epi="dgelu", aux="h16", bias=True), dict(rps=10, scale_zero=True, res="f32", bias=True),
                dict(res="h16", res_row_mod=20, c="h16"), dict(rps=65, res="f32"), dict(rps=1, bias=True),
                dict(res="f32", res_up=UP, bias=True), dict(res="h16", res_up=UP, rps=100, c="h16")]


def generic_cases():
    """gemm_kernel: both compute types x three layouts x four shapes (algo 2 keeps the fp32 problems off the tiny kernel; odd leading
    dimensions keep the 16-bit ones off gemm2), the scalar staging path (odd ld, A off by one element) and the vector one, every
    epilogue, atomic and deterministic split-K with split_k = 3 at K = 40 (two slabs result) and K = 200 (three)."""
    t = []
    for layout, f32 in itertools.product(LAYOUTS, (True, False)):
        tag = f"generic-{layout}-{'f32' if f32 else 'h16'}"
        for i, (M, N, K) in enumerate(GENERIC_SHAPES):
            if f32:
                kw = dict(F32C, algo=2, pad=(4, 1, 4, 4)[i], mis={"A": 1} if i == 3 else None)
                if i == 1:
                    kw["a"] = "h16"                # 16-bit operand under fp32 compute: upcast, not rounded
            else:
                # pad 1: odd leading dimensions (scalar staging); N = 97 / K = 33 keep gemm2 away at 16-byte aligned rows (vector staging)
                kw = dict(a=("h16", "f32")[i % 2], b=("f32", "h16")[(i // 2) % 2], c=("f32", "h16")[i % 2], pad=(1, 8, 1, 7)[i],
                          mis={"A": 1} if i == 0 else None)
            t.append((f"{tag}-{M}x{N}x{K}", name_gemm(layout, f32), case(layout, M, N, K, **kw)))
    for f32 in (True, False):
        for j, e in enumerate(GENERIC_EPIS):
            layout = LAYOUTS[j % 3]
            kw = dict(F32C, algo=2, pad=4) if f32 else dict(a="h16", b="f32", c="f32", pad=8)
            kw.update(e)
            t.append((f"generic-epi{j}-{layout}-{'f32' if f32 else 'h16'}", name_gemm(layout, f32),
                      case(layout, 256 if "res_up" in e else 65, 97, 40, **kw)))
        for layout, K, det in itertools.product(LAYOUTS, (40, 200), (False, True)):
            kw = dict(F32C, algo=2, pad=4) if f32 else dict(a="h16", b="h16", c="f32", pad=1)
            if det:
                kw.update(dict(bias=True, epi="gelu", aux="f32") if K == 40 else dict(bias=True, rps=10, res="f32", c="f32" if f32 else "h16"))
            else:
                kw.update(bias=True)
            t.append((f"generic-split3-{'det' if det else 'atomic'}-{layout}-K{K}-{'f32' if f32 else 'h16'}", name_gemm(layout, f32),
                      case(layout, 65, 97, K, split=3, det=det, **kw)))
    return both_kinds(t)


# epilogues dealt over the 21 instantiations of gemm2_kernel (M = tile rows + 24: whole 64-row groups and a ragged last one)
G2_EPIS = [dict(), dict(bias=True, epi="gelu", aux="h16"), dict(epi="dgelu", aux="h16"), dict(RES, bias=True, rps=100, scale_zero=True),
           dict(res="h16", res_row_mod=40), dict(c="f32", bias=True, epi="gelu", aux="f32"), dict(RES, rps=1), dict(RES, rps=-1, bias=True),
           dict(c="f32", epi="dgelu", aux="f32", bias=True), dict(bias=True, epi="gelu"), dict(RES, res_row_mod=72, rps=100),
           dict(c="f32", bias=True, epi="gelu", aux="h16")]    # (fp32 C beside a 16-bit aux: gelu_fast where no 16-bit rounding of C hides it)


def gemm2_cases():
    """gemm2_kernel: every dtype / layout combination at forced tile rows 64 / 128 / 256, M = rows + 24 (a ragged last row tile),
    N = 136 (a ragged 128-column tile), K = 8, 64, 72, 128 and the epilogues dealt over them; then, on 64- and 128-row tiles: the fused
    colsum (TN) unsplit and with deterministic split-K, atomic split-K, res_up, the whole-line residual epilogue on whole 64-row groups
    (res_lines) with rows_per_scale 1 / 100 / M and one scale 0, and the automatic tile."""
    t, i = [], 0
    for layout, a, b in G2_COMBOS:
        for rows in (64, 128, 256):
            if rows == 256 and a == "f32":
                continue
            M, K = rows + 24, (8, 64, 72, 128)[i % 4]
            e = dict(G2_EPIS[i % len(G2_EPIS)])
            if e.get("rps") == -1:
                e["rps"] = M
            t.append((f"gemm2-{layout}-{a}-{b}-rows{rows}-K{K}-epi{i % len(G2_EPIS)}", name_gemm2(layout, a, b, rows),
                      case(layout, M, 136, K, a=a, b=b, tile_rows=rows, **e)))
            i += 1
    for a in ("h16", "f32"):
        for rows in (64, 128):
            t.append((f"gemm2-colsum-{a}-rows{rows}", name_gemm2("TN", a, "h16", rows),
                      case("TN", rows + 24, 136, 72, a=a, c="f32", colsum=True, tile_rows=rows)))
            t.append((f"gemm2-colsum-det-{a}-rows{rows}", name_gemm2("TN", a, "h16", rows),
                      case("TN", rows + 24, 136, 320, a=a, c="f32", colsum=True, split=3, det=True, tile_rows=rows)))
            t.append((f"gemm2-atomic-{a}-rows{rows}", name_gemm2("TN", a, "h16", rows),
                      case("TN", rows + 24, 136, 320, a=a, c="f32", split=3, bias=True, tile_rows=rows)))
    for rows in (64, 128):
        t.append((f"gemm2-res_up-rows{rows}", name_gemm2("NT", "h16", "h16", rows),
                  case("NT", 256, 136, 64, bias=True, res_up=UP, tile_rows=rows, **RES)))
        t.append((f"gemm2-res_up-h16-rows{rows}", name_gemm2("NN", "h16", "f32", rows),
                  case("NN", 256, 136, 72, b="f32", res="h16", res_up=UP, rps=100, tile_rows=rows)))
        for rps in (1, 100, 2 * rows):
            t.append((f"gemm2-res_lines-rows{rows}-rps{rps}", name_gemm2("NT", "h16", "h16", rows),
                      case("NT", 2 * rows, 136, 128, bias=True, rps=rps, scale_zero=True, tile_rows=rows, **RES)))
        t.append((f"gemm2-det-NT-rows{rows}", name_gemm2("NT", "h16", "f32", rows),
                  case("NT", rows + 24, 136, 320, b="f32", split=3, det=True, bias=True, epi="gelu", aux="h16", tile_rows=rows)))
    t.append(("gemm2-auto-tile", name_gemm2("NT", "h16", "h16", 64), case("NT", 100, 136, 72, bias=True, **RES)))
    return both_kinds(t)


G3_EPIS = [dict(), dict(bias=True, epi="gelu", aux="h16"), dict(RES, bias=True, rps=100, scale_zero=True), dict(epi="dgelu", aux="h16"),
           dict(res="h16", res_row_mod=24, bias=True), dict(c="f32", bias=True, epi="gelu", aux="f32"), dict(c="f32", bias=True, epi="gelu", aux="h16")]


def gemm3_cases():
    """gemm3_kernel<MT, S> through algo 300 + 10 MT + S: K = 16, 48, 64, 96, 64 S, 64 S + 16 (fewer k-tiles than ring stages, every
    k-tail: K % 64 = 16, 32, 48), M = 40 (less than one tile) and 64 MT + 8, N = 136; the residual-stream epilogue of the 64-row form on whole tiles; and
    algo 1312: 33 x 8 = 264 tiles of 64 x 128 on 256 workgroups."""
    t, i = [], 0
    for mt, s in itertools.product((1, 2, 4), (2, 3, 4)):
        if mt == 4 and s == 4:
            continue
        for K in (16, 48, 64, 96, 64 * s, 64 * s + 16):
            M = 40 if (i + i // 6) % 2 else 64 * mt + 8
            t.append((f"gemm3-{mt}-{s}-M{M}-K{K}-epi{i % len(G3_EPIS)}", name_gemm3(mt, s),
                      case("NT", M, 136, K, algo=300 + 10 * mt + s, **G3_EPIS[i % len(G3_EPIS)])))
            i += 1
    for s in (2, 3, 4):
        t.append((f"gemm3-1-{s}-residual-stream", name_gemm3(1, s), case("NT", 128, 256, 64 * s + 16, algo=310 + s, bias=True, rps=32, **RES)))
    t.append(("gemm3-1-2-more-tiles-than-workgroups", name_gemm3(1, 2), case("NT", 64 * 33, 1024, 16, algo=1312, bias=True)))
    return both_kinds(t)


def _g4_form_kw(form, second):
    """Keyword sets that make gemm4_form answer `form` on whole tiles."""
    return {1: dict(bias=True), 2: dict(bias=True, epi="gelu", aux=None if second else "h16", gelu_dt="h16"), 3: dict(),
            4: dict(epi="dgelu", aux="h16"), 5: dict(RES, rps=32) if second else dict(RES, bias=True)}[form]


# FORM 0 on whole tiles: the epilogues forms 1 - 5 do not take
G4_FORM0 = [dict(res="h16", bias=True), dict(RES, res_row_mod=-1), dict(bias=True, epi="gelu", aux="f32"), dict(rps=32, bias=True),
            dict(c="f32", bias=True, epi="gelu", aux="h16")]


def gemm4_cases():
    """gemm4_kernel through algo 400 + variant: forms 1 - 5 on 2 x 1 whole tiles at K = 64 (one k-tile on the ring) and K = 64 (S + 1);
    FORM 2 with aux == NULL; FORM 5 with and without a bias and with a row scale every 32 and 100 rows; FORM 0 on ragged M and N and on
    whole tiles with a 16-bit residual, res_row_mod, fp32 aux, a row scale, fp32 C beside a 16-bit aux; the variants without forms on ragged and whole tiles; and
    one case per tile shape with 257 tiles on the 256 workgroups of algo 1400 + variant."""
    t = []
    for v, (wm, mt, nt, s, forms, np_) in G4.items():
        BM, BN = g4_tile(v)
        ragged = case("NT", BM + 40, BN + 8, 64 * (s + 1), algo=400 + v, bias=True, epi="gelu", aux="h16")
        t.append((f"gemm4-{v}-form0-ragged", name_gemm4(v, 0), ragged))
        if forms:
            for form, second in itertools.product((1, 2, 3, 4, 5), (False, True)):
                t.append((f"gemm4-{v}-form{form}-K{64 * (s + 1) if second else 64}", name_gemm4(v, form),
                          case("NT", 2 * BM, BN, 64 * (s + 1) if second else 64, algo=400 + v, **_g4_form_kw(form, second))))
            t.append((f"gemm4-{v}-form5-rps100", name_gemm4(v, 5), case("NT", 2 * BM, 2 * BN, 64, algo=400 + v, bias=True, rps=100, **RES)))
            for j, e in enumerate(G4_FORM0):
                e = dict(e)
                if e.get("res_row_mod") == -1:
                    e["res_row_mod"] = BM // 2 + 8
                t.append((f"gemm4-{v}-form0-whole-{j}", name_gemm4(v, 0), case("NT", 2 * BM, BN, 128, algo=400 + v, **e)))
        else:
            t.append((f"gemm4-{v}-form0-whole", name_gemm4(v, 0), case("NT", 2 * BM, BN, 64, algo=400 + v, bias=True)))
            t.append((f"gemm4-{v}-form0-residual", name_gemm4(v, 0), case("NT", BM, 2 * BN, 64 * (s + 1), algo=400 + v, rps=100, **RES)))
    for v in (2, 12, 22, 32, 62, 42, 52, 72, 83, 84):          # one per tile shape
        BM, BN = g4_tile(v)
        t.append((f"gemm4-{v}-more-tiles-than-workgroups", name_gemm4(v, 1 if G4[v][4] else 0),
                  case("NT", 257 * BM, BN, 64, algo=1400 + v, bias=True)))
    return both_kinds(t)


def _g5_form_kw(form, i):
    return {0: dict(bias=True), 1: dict(bias=True, epi="gelu", aux="h16") if i % 2 == 0 else dict(bias=True, epi="gelu"),
            2: dict(epi="dgelu", aux="h16"), 3: dict(RES, bias=True, rps=(32, 0)[i % 2]), 4: dict(c="f32", bias=True)}[form]


def _g5_problem(kch, nb, wide):
    """(N, algo) that reach gemm5_kernel<kch, nb, .>; wide: twice the narrowest N."""
    K = 96 * kch
    if nb == 6:
        return (384 if wide else 192), (506 if K == 192 else 500)
    if K == 96:
        return (288 if wide else 96), 500          # N % 192 != 0
    return (192 if wide else 96), (503 if K == 192 else 500)


def gemm5_cases():
    """gemm5_kernel<KCH, NB, W, form> through algo 500 / 503 / 506: every instantiation at M = 32 (one unit: all waves but one find
    nothing to do) and M = 96, N = 96 and 192 (NB 3) resp. 192 and 384 (NB 6); every form-3 kernel at M = 160 with rows_per_scale 32
    (five scales, one of them 0) and 64 (three scales); and per
    (KCH, NB, W) one pass of the persistent grid + 32 rows (form 3 at K = 96, N = 768: 8192 + 32, and two passes + 32)."""
    t, i = [], 0
    for (kch, nb, w), forms in G5.items():
        for form in forms:
            for M, wide in ((32, False), (96, True)):
                N, algo = _g5_problem(kch, 3 if form == 3 else nb, wide)
                if form == 3 and nb != 3:
                    continue
                t.append((f"gemm5-{kch}-{nb}-{w}-form{form}-M{M}-N{N}", name_gemm5(kch, nb, w, form),
                          case("NT", M, N, 96 * kch, algo=algo, **_g5_form_kw(form, i))))
                i += 1
        if 3 in forms:                            # every form-3 kernel with rows_per_scale 32 and 64 at an M that holds several scales
            N, algo = _g5_problem(kch, 3, False)
            for rps in (32, 64):
                t.append((f"gemm5-{kch}-{nb}-{w}-form3-M160-rps{rps}", name_gemm5(kch, nb, w, 3),
                          case("NT", 160, N, 96 * kch, algo=algo, bias=True, rps=rps, scale_zero=rps == 32, **RES)))
    one = g5_pass_rows(768, 3, 8)
    assert one == 8192
    for M in (one + 32, 2 * one + 32):
        t.append((f"gemm5-1-3-8-form3-M{M}-N768", name_gemm5(1, 3, 8, 3), case("NT", M, 768, 96, algo=500, bias=True, rps=64, **RES)))
    t.append((f"gemm5-2-3-8-form0-pass", name_gemm5(2, 3, 8, 0), case("NT", g5_pass_rows(768, 3, 8) + 32, 768, 192, algo=503, bias=True)))
    t.append((f"gemm5-4-3-6-form1-pass", name_gemm5(4, 3, 6, 1),
              case("NT", g5_pass_rows(384, 3, 6) + 32, 384, 384, algo=500, bias=True, epi="gelu", aux="h16")))
    t.append((f"gemm5-2-6-6-form2-pass", name_gemm5(2, 6, 6, 2), case("NT", g5_pass_rows(768, 6, 6) + 32, 768, 192, algo=506, epi="dgelu", aux="h16")))
    t.append((f"gemm5-1-6-8-form4-pass", name_gemm5(1, 6, 8, 4), case("NT", g5_pass_rows(768, 6, 8) + 32, 768, 96, algo=500, c="f32", bias=True)))
    return both_kinds(t)


def finish_cases():
    """splitk_finish_kernel<VEC, SL>: VEC 4 (N % 4 == 0) / 1, SL 16 (>= 16 slabs, < 16384 output vectors) / 4 (>= 4 slabs, < 131072)
    / 1, behind gemm_kernel (fp32 compute, k-tiles of 32) -- without an activation, so that the pass is additions only and an exact-order
    fp32 emulation gives its bits.  ((id, (VEC, SL)), name, case)."""
    t = []
    for N, (split, K) in itertools.product((96, 97), ((3, 96), (5, 160), (17, 544))):
        c = case("NT", 40, N, K, split=split, det=True, bias=N == 96, algo=2, pad=4, kind="plain", seed=N + split, **F32C)
        t.append((f"finish-N{N}-split{split}", name_gemm("NT", True), c))
    t.append(("finish-h16-out", name_gemm("NT", True), case("NT", 40, 96, 544, split=17, det=True, bias=True, algo=2, pad=4, kind="offset",
                                                              seed=5, a="f32", b="f32", c="h16", compute="f32")))
    return t


TABLES = {"tiny": tiny_cases, "generic": generic_cases, "gemm2": gemm2_cases, "gemm3": gemm3_cases, "gemm4": gemm4_cases, "gemm5": gemm5_cases,
          "finish": finish_cases}


def all_cases():
    return [e for f in TABLES.values() for e in f()]


# the child on the fp16 library: one exact and one random case per family, every gemm5 form, gemm4 forms 2, 4 and 5, and the two value
# sets only fp16 has
def fp16_cases():
    pick = {"tiny": ("tiny-NT-K17-bias",), "generic": ("generic-NN-h16-65x97x40", "generic-epi2-TN-h16"),
            "gemm2": ("gemm2-NT-h16-h16-rows128-K64-epi1", "gemm2-colsum-det-h16-rows64"), "gemm3": ("gemm3-1-3-M40-K64-epi1",),
            "gemm4": ("gemm4-63-form2-K64", "gemm4-63-form4-K256", "gemm4-63-form5-K256", "gemm4-33-form0-ragged"),
            "gemm5": tuple(f"gemm5-2-3-8-form{f}-M96-N192" for f in range(5))}
    out = []
    for fam, ids in pick.items():
        table = TABLES[fam]()
        for cid in ids:
            hit = [e for e in table if e[0].rsplit("-", 1)[0] == cid]
            assert len(hit) == 2, (cid, [e[0] for e in table][:8])
            out += hit
    edge = {"gemm_kernel": ("generic", case("NN", 65, 97, 40, a="f32", b="h16", c="h16", pad=1), name_gemm("NN", False)),
            "gemm2": ("gemm2", case("NT", 152, 136, 72, tile_rows=128), name_gemm2("NT", "h16", "h16", 128)),
            "gemm4": ("gemm4", case("NT", 256, 192, 256, algo=463), name_gemm4(63, 3)),
            "gemm5": ("gemm5", case("NT", 96, 192, 192, algo=503), name_gemm5(2, 3, 8, 0))}
    for kind in ("big", "subnormal"):
        for fam, (_, c, name) in edge.items():
            out.append((f"{fam}-{kind}", name, dict(c, kind=kind, seed=11)))
    return out


# the child with the library's switches set: the kernels only a switch reaches under algo 0, one case each
SWITCH_ENV = {"CSTS_GEMM4_T64": "3", "CSTS_GEMM5_K384": "1", "CSTS_GEMM5_WIDE192": "1", "CSTS_GEMM_RES_LINES": "0"}


def switch_cases():
    return [("switch-gemm4-t64", name_gemm4(73, 2), case("NT", 2048, 384, 384, bias=True, epi="gelu", aux="h16", kind="offset", seed=3)),
            ("switch-gemm4-t64-res", name_gemm4(73, 5), case("NT", 2048, 384, 384, bias=True, kind="exact", seed=4, **RES)),
            ("switch-gemm5-k384", name_gemm5(4, 3, 6, 0), case("NT", 16384, 96, 384, bias=True, kind="offset", seed=5)),
            ("switch-gemm5-wide192", name_gemm5(2, 6, 6, 0), case("NT", 16384, 192, 192, bias=True, kind="exact", seed=6)),
            ("switch-gemm2-res-lines-0", name_gemm2("NT", "h16", "h16", 128),
             case("NT", 256, 136, 128, bias=True, rps=100, tile_rows=128, kind="offset", seed=7, **RES))]
