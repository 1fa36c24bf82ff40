"""Raw C-ABI harness for the attention core of csts_amd/csrc/attention.hip (csts_attn_fwd, csts_attn_bwd, csts_attn_bwd_workspace,
csts_attn_probs) against the float64 reference of tests/attention_core_reference.py.  Shared by tests/test_gpu_attention_core.py
(bf16 library, default switches) and tests/attention_worker.py (child processes: all switches off, CSTS_ATTN_DQ_FAST=4, the fp16
library); not a test module itself.  Region, the guard bands and the NaN patterns are those of tests/stencil_raw.py.

Operand placement, the way ops.py hands the kernels views of wider buffers: Q is slot 0 of a (B, Nq, 3C) buffer, K and V are the two
slots of one (B, Nk, 2C) buffer (Nk == 8: slots 1 and 2 of a 3C-wide one), O and dO are dense, dQ goes to slot 0 of a 3C-wide buffer,
dK and dV to the two slots of one 2C-wide buffer, LSE and delta are fp32 (B, H, Nq), the workspace is exactly
csts_attn_bwd_workspace bytes.  Every buffer sits between guard bands, every input buffer is NaN outside its own slots, every output
region is pre-filled with a NaN pattern.  After a call every owned element must be finite, every guard / foreign slot bit-intact,
and delta all pre-fill after a one-pass call, all finite after a two-kernel call.

The backward is run on O_in / LSE_in of the REFERENCE (rounded to the storage type / fp32), never on the forward kernel's outputs.

Bars (u = 2^-24; u16 = 2^-8 bf16, 2^-11 fp16; u_out = 0 / u16 for fp32 / 16-bit outputs; fp16 outputs add 2^-25; A, A_z: the
magnitudes of the reference):
  delta             |err| <= (hd + 1) u A_delta                                   DERIVED: the record holds ratio = |err| / bar
  LSE               |err| <= C_L u (1 + |LSE| + A_z)
  probs             |err| <= C_P u (1 + |LSE_in| + A_z) P + 2^-126
  O, dQ, dK, dV     |err| <= C eps A + u_out |ref|,  eps = u (1 + A_z) in fp32 mode, u16 in 16-bit mode (P, P^T and dS are rounded
                    to 16 bits before the second products); for dK / dV, whose elements sum over the queries, A_z is the largest
                    of the (batch, head)
Every element is held.  For the measured bars a record holds `need`: the smallest constant at which every element passes, and the
index of the element that needs it with the tile / wave / lane / split it falls in; the caller compares `need` with its constant."""
import ctypes as C

import torch

from csts_amd import lib as L
import attention_core_reference as AR
from stencil_raw import GUARD, PREFILL, SENT, Region, _sx, _unravel, rand, stream   # noqa: F401  (re-exported for the callers)

U = AR.U
INF = float("inf")


def store_key(dk):
    """ "f32" | "h16" -> the storage type of this process: "f32" | "bf16" | "fp16"."""
    return "f32" if dk == "f32" else L.HALF


def to_rows(t):
    B, H, N, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * hd)


def from_rows(t, H):
    B, N, Cc = t.shape
    return t.reshape(B, N, H, Cc // H).permute(0, 2, 1, 3)


def f32_region(n, dev):
    return Region(1, 1, n, torch.float32, dev, ts=(n + 7) // 8 * 8)


def prefilled(r):
    """Every owned element still holds the pre-fill pattern."""
    return bool((r.ibuf[r.mask] == _sx(PREFILL[r.es], r.es)).all())


def _set3(arr, bs, ts, hd):
    arr[0], arr[1], arr[2] = bs, ts, hd


# ------------------------------------------------------------------------------------------------------------ records
def _worst(r, shape):
    r = r.nan_to_num(nan=INF, posinf=INF)
    i = int(r.argmax())
    return float(r.flatten()[i]), _unravel(i, shape)


def need(got, ref, denom, slack):
    """The smallest constant c with |got - ref| <= c denom + slack for every element (an excess where denom == 0 counts as
    infinite, as does a non-finite element) and the index of the element that needs it."""
    err = (got - ref).abs()
    excess = (err - slack).clamp_min(0.0)
    excess = torch.where(torch.isfinite(got), excess, torch.full_like(excess, INF))
    r = torch.where(denom > 0, excess / denom, torch.where(excess > 0, torch.full_like(excess, INF), torch.zeros_like(excess)))
    return _worst(r, got.shape)


def where_query(idx, plan):
    b, h, i = idx[:3]
    s = f"b {b} head {h} query {i}: 128-row tile {i // 128} wave {i % 128 // 32} lane {i % 32}"
    if plan is not None:
        s += f", split {i // plan['q_chunk']} of {plan['nsplit']} (row {i % plan['q_chunk']} of its chunk)"
    return s + (f", channel {idx[3]} (32-column block {idx[3] // 32})" if len(idx) > 3 else "")


def where_key(idx, hd, Nk):
    b, h, k, d = idx
    t = 64 if hd == 96 else 32
    return (f"b {b} head {h} key {k}: 128-key block {k // 128} wave {k % 128 // 32} lane {k % 32}, {t}-key tile {k // t} "
            f"(key {k % t} of {min(t, Nk - k // t * t)} live), channel {d}")


def _rec(name, val, idx, where, got, ref, key="need"):
    return {"name": name, key: val, "at": list(idx), "where": where, "got": float(got[idx]), "ref": float(ref[idx])}


# ------------------------------------------------------------------------------------------------------------ one problem
class Problem:
    """The operands of one reference case on the device and the three calls."""

    def __init__(self, ref, dev):
        self.ref, self.dev = ref, dev
        self.B, self.H, self.Nq, self.Nk = ref["shape"]
        self.hd, self.dt = ref["hd"], ref["store"]
        self.C = self.H * self.hd
        self.es = torch.empty(0, dtype=self.dt).element_size()
        self.u16 = AR.U16[self.dt]
        self.sub = 2.0 ** -25 if self.dt == torch.float16 else 0.0
        self.Q = Region(self.B, self.Nq, self.C, self.dt, dev, ts=3 * self.C, off=0, pad=24).load(to_rows(ref["q"]).to(dev))
        self.lib = L.load()

    # operands
    def kv(self, v):
        """K and V in the two slots of one 2C-wide buffer; Nk == 8: in slots 1 and 2 of a 3C-wide buffer."""
        three = self.Nk == 8
        r = Region(self.B, self.Nk, 2 * self.C, self.dt, self.dev, ts=(3 if three else 2) * self.C, off=self.C if three else 0, pad=24)
        return r.load(torch.cat([to_rows(self.ref["k"]), to_rows(v)], dim=-1).to(self.dev))

    def dense(self, data=None):
        r = Region(self.B, self.Nq, self.C, self.dt, self.dev)
        return r.arm() if data is None else r.load(to_rows(data).to(self.dev))

    def stat(self, data=None):
        r = f32_region(self.B * self.H * self.Nq, self.dev)
        return r.arm() if data is None else r.load(data.reshape(1, 1, -1).float().to(self.dev))

    def args(self, KV, O, LSE, dO=None, delta=None, dQ=None, dKV=None, masked=True):
        a = L.AttnArgs()
        a.Q, a.K, a.V = self.Q.ptr(), KV.ptr(), KV.ptr() + self.C * self.es
        a.O, a.LSE = O.ptr(), LSE.ptr()
        a.dtype, a.B, a.H, a.Nq, a.Nk, a.head_dim = (L.F32 if self.dt == torch.float32 else L.BF16), self.B, self.H, self.Nq, self.Nk, self.hd
        _set3(a.q_strides, self.Q.bs, self.Q.ts, self.hd)
        _set3(a.k_strides, KV.bs, KV.ts, self.hd)
        _set3(a.v_strides, KV.bs, KV.ts, self.hd)
        _set3(a.o_strides, O.bs, O.ts, self.hd)
        if dO is not None:
            a.dO, a.delta, a.dQ, a.dK, a.dV = dO.ptr(), delta.ptr(), dQ.ptr(), dKV.ptr(), dKV.ptr() + self.C * self.es
            _set3(a.do_strides, dO.bs, dO.ts, self.hd)
            _set3(a.dq_strides, dQ.bs, dQ.ts, self.hd)
            _set3(a.dk_strides, dKV.bs, dKV.ts, self.hd)
            _set3(a.dv_strides, dKV.bs, dKV.ts, self.hd)
        a.scale = self.ref["scale"]
        if masked and self.ref["mask"] is not None:
            a.mask_mode, (a.mask_T, a.mask_HW) = L.MASK_SPATIAL, self.ref["mask"]
        return a

    def plan(self):
        return AR.plan(self.B, self.H, self.Nq, self.Nk, self.hd, self.dt != torch.float32, self.ref["mask"] is not None, AR.env_of())

    def bwd_operands(self):
        """Fresh buffers of one backward call: KV, O_in, LSE_in, dO, delta, dQ, dKV, workspace and the arguments."""
        KV, O, LSE = self.kv(self.ref["v"]), self.dense(self.ref["o_in"]), self.stat(self.ref["lse_in"])
        dO, delta = self.dense(self.ref["do"]), self.stat()
        dQ = Region(self.B, self.Nq, self.C, self.dt, self.dev, ts=3 * self.C, off=0, pad=24).arm()
        dKV = Region(self.B, self.Nk, 2 * self.C, self.dt, self.dev, ts=2 * self.C, pad=24).arm()
        a = self.args(KV, O, LSE, dO, delta, dQ, dKV)
        wsz = int(self.lib.csts_attn_bwd_workspace(C.byref(a)))
        ws = f32_region(max(wsz // 4, 1), self.dev).arm()
        return {"KV": KV, "O": O, "LSE": LSE, "dO": dO, "delta": delta, "dQ": dQ, "dKV": dKV, "ws": ws, "wsz": wsz, "a": a}

    # bars
    def _eps_q(self):                                         # per query row, (B, H, Nq, 1)
        return (U * (1 + self.ref["A_z"]))[..., None] if self.dt == torch.float32 else torch.full((1, 1, 1, 1), self.u16, dtype=torch.float64)

    def _eps_k(self):                                         # per (batch, head), (B, H, 1, 1)
        return (U * (1 + self.ref["A_z"].amax(-1)))[..., None, None] if self.dt == torch.float32 else torch.full((1, 1, 1, 1), self.u16, dtype=torch.float64)

    def _out(self, name, got, ref, A, eps, where):
        val, idx = need(got, ref, eps * A, self.u16 * ref.abs() + self.sub)
        return _rec(name, val, idx, where(idx), got, ref)

    # the calls
    def fwd(self):
        KV, O, LSE = self.kv(self.ref["v_fwd"]), self.dense(), self.stat()
        a = self.args(KV, O, LSE)
        L.check(self.lib.csts_attn_fwd(C.byref(a), stream()), "csts_attn_fwd")
        torch.cuda.synchronize()
        r = self.ref
        got_o = from_rows(O.view().cpu().double(), self.H)
        got_l = LSE.view().cpu().double().reshape(self.B, self.H, self.Nq)
        val, idx = need(got_l, r["LSE"], U * (1 + r["LSE"].abs() + r["A_z"]), 0.0)
        self.raw_fwd = (O.ibuf.clone(), LSE.ibuf.clone())
        return {"O": self._out("O", got_o, r["O"], r["A_O"], self._eps_q(), lambda i: where_query(i, None)),
                "LSE": _rec("LSE", val, idx, where_query(idx, None), got_l, r["LSE"]),
                "fwd_finite": O.finite() and LSE.finite(), "fwd_guards": O.guards_ok() and LSE.guards_ok()}

    def bwd(self):
        o = self.bwd_operands()
        L.check(self.lib.csts_attn_bwd(C.byref(o["a"]), o["ws"].ptr(), o["wsz"], stream()), "csts_attn_bwd")
        torch.cuda.synchronize()
        r, pl = self.ref, self.plan()
        dq = from_rows(o["dQ"].view().cpu().double(), self.H)
        dkv = o["dKV"].view().cpu().double()
        dk, dv = from_rows(dkv[..., :self.C], self.H), from_rows(dkv[..., self.C:], self.H)
        wq = lambda i: where_query(i, pl)                                         # noqa: E731
        wk = lambda i: where_key(i, self.hd, self.Nk)                             # noqa: E731
        out = {"dQ": self._out("dQ", dq, r["dQ"], r["A_dQ"], self._eps_q(), wq),
               "dK": self._out("dK", dk, r["dK"], r["A_dK"], self._eps_k(), wk),
               "dV": self._out("dV", dv, r["dV"], r["A_dV"], self._eps_k(), wk),
               "plan": pl, "ws_bytes": o["wsz"],
               "bwd_finite": o["dQ"].finite() and o["dKV"].finite(),
               "bwd_guards": all(o[k].guards_ok() for k in ("dQ", "dKV", "ws", "delta"))}
        if pl["path"] == "one-pass":
            out["delta_state"] = "prefill" if prefilled(o["delta"]) else "touched"
        else:
            got_d = o["delta"].view().cpu().double().reshape(self.B, self.H, self.Nq)
            out["delta_state"] = "finite" if o["delta"].finite() else "non-finite"
            val, idx = need(got_d, r["delta"], (self.hd + 1) * U * r["A_delta"], 0.0)
            out["delta"] = _rec("delta", val, idx, wq(idx), got_d, r["delta"], key="ratio")
        self.raw_bwd = (o["dQ"].ibuf.clone(), o["dKV"].ibuf.clone())
        return out

    def probs(self, q=None):
        KV, O, LSE = self.kv(self.ref["v"]), self.dense(), self.stat(self.ref["lse_in"])
        n = self.B * self.H * self.Nq * self.Nk
        P = f32_region(n, self.dev).arm()
        a = self.args(KV, O, LSE)
        L.check(self.lib.csts_attn_probs(C.byref(a), P.ptr(), stream()), "csts_attn_probs")
        torch.cuda.synchronize()
        return {"probs": probs_record(P, self.ref, (self.B, self.H, self.Nq, self.Nk)),
                "probs_finite": P.finite(), "probs_guards": P.guards_ok() and prefilled(O)}


def probs_record(P, ref, shape):
    got = P.view().cpu().double().reshape(shape)
    pin = ref["P_in"]
    val, idx = need(got, pin, U * (1 + ref["lse_in"].abs() + ref["A_z"])[..., None] * pin, 2.0 ** -126)
    rec = _rec("probs", val, idx, where_query(idx[:3], None) + f", key {idx[3]}", got, pin)
    rec["masked_exact_zero"] = bool((got[pin == 0] == 0).all())
    return rec


def run_case(name, hd, dk, dev, variant=""):
    """fwd, bwd and (where the case has them) probs of one run -> the records and flags of all three."""
    ref = AR.reference(name, hd, store_key(dk), variant)
    pr = Problem(ref, dev)
    out = {"case": f"{name}{variant} hd{hd} {store_key(dk)}", "store": store_key(dk)}
    out.update(pr.fwd())
    out.update(pr.bwd())
    if AR.CASES[name][7]:
        out.update(pr.probs())
    return out, pr


def run_probs_cap(dev):
    """csts_attn_probs alone at PROBS_CAP (fp32): more elements than one trip of its 4096 x 256 threads."""
    B, H, Nq, Nk, hd = AR.PROBS_CAP
    r = AR.probs_cap_reference()
    ref = {"shape": (B, H, Nq, Nk), "hd": hd, "store": torch.float32, "q": r["q"], "k": r["k"], "v": torch.zeros(B, H, Nk, hd),
           "lse_in": r["lse_in"], "mask": None, "scale": r["scale"], "P_in": r["P_in"], "A_z": r["A_z"]}
    out = Problem(ref, dev).probs()
    out.update({"case": "probs_cap", "store": "f32"})
    return out


# ------------------------------------------------------------------------------------------------------------ verdicts
MEASURED = ("O", "LSE", "dQ", "dK", "dV", "probs")


def violations(res, consts):
    """Every reason this run misses: a flag, the derived delta bar (ratio <= 1), a measured bar (need <= consts[(output, mode)],
    mode "f32" | "h16")."""
    mode = "f32" if res["store"] == "f32" else "h16"
    bad = [k for k in ("fwd_finite", "fwd_guards", "bwd_finite", "bwd_guards", "probs_finite", "probs_guards") if k in res and not res[k]]
    if "plan" in res:
        want = "prefill" if res["plan"]["path"] == "one-pass" else "finite"
        if res["delta_state"] != want:
            bad.append(f"delta {res['delta_state']}, expected {want}")
        if res["ws_bytes"] != res["plan"]["ws"]:
            bad.append(f"workspace {res['ws_bytes']} bytes, the plan implies {res['plan']['ws']}")
    if "delta" in res and not res["delta"]["ratio"] <= 1.0:
        bad.append(res["delta"])
    for k in MEASURED:
        if k in res and not res[k]["need"] <= consts[(k, mode)]:
            bad.append(res[k])
    if "probs" in res and not res["probs"]["masked_exact_zero"]:
        bad.append("a masked probability is not exactly 0")
    return bad


def summary(res):
    parts = [f"{k} {res[k]['need']:.3g}" for k in MEASURED if k in res] + ([f"delta/bar {res['delta']['ratio']:.3g}"] if "delta" in res else [])
    return f"[{res['case']}] " + "  ".join(parts) + (f"  ({res['plan']['path']}, nsplit {res['plan']['nsplit']})" if "plan" in res else "")
