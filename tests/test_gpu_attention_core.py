"""The attention core of csts_amd/csrc/attention.hip, element by element against float64 (tests/attention_core_reference.py), through
raw C-ABI calls on operands inside wider buffers (tests/attention_raw.py, which states the placement, the guards and the bars):
csts_attn_fwd (O, LSE), csts_attn_bwd (delta where written, dQ, dK, dV; handed O_in / LSE_in of the reference, never the forward
kernel's outputs) and csts_attn_probs.  tests/test_attention_core_reference_host.py holds the plan restatement that lists which case
reaches which kernel instantiation, and asserts that the cases below reach all of them.

Measured on MI355X over every in-process run, the three children and both libraries, two sets of seeds (the worst `need` = the
smallest constant at which every element passes; the committed constants, about 4x, are CONSTS below with the worst case named):
              LSE (C_L)   probs (C_P)   O       dQ      dK      dV
  fp32        2.44        2.04          2.23    0.285   0.177   1.76
  bf16        1.05        1.02          0.82    0.158   0.131   0.72
  fp16        1.10        1.57          0.40    0.085   0.066   0.41
Derived bar, delta (ratio |err| / ((hd + 1) u A_delta) <= 1): worst 0.023 (fp32), 0.010 (bf16), 0.022 (fp16).  The one-pass
backward leaves delta as pre-filled in every run; the two-kernel backward writes every element.
Wall time: 85 tests in 12 s, of which the three children take 7 s together (2.1 - 2.3 s each); no test above 1.3 s.

Mutation check (scratch builds of attention.hip loaded through CSTS_HIP_LIB, one arithmetic-only change each, no new address and no
longer loop, each run once).  Of the tests here, on MI355X, each mutant fails (in brackets: how many of the 32 attention tests of
tests/test_gpu_ops.py fail on the same library):
  29  attn_fwd_kernel counts key Nk - 1 as dead in its per-element test                       (test_case 27, generic child 2)   [22]
  11  attn_fwd_kernel's rescale skips the last 32-column block of O                           (test_case 10, generic child 1)   [1]
   2  attn_fwd_fast_kernel's rescale skips the last 32-column block of O                      (test_case[staircase*-h16])       [0]
  34  attn_dq_kernel leaves the half-wave shuffle-add out of delta                            (test_case 28, generic child 6)   [20]
   7  attn_dq_fast_kernel does the same                                                       (test_case 5, dq4 child 2)        [7]
   1  attn_bwd_fused_kernel counts the last live query of a ragged chunk as dead in part A    (test_case[fused_ragged])         [3]
  18  attn_dkv_kernel (SLOW) does the same with qend - 1                                      (test_case 18)                    [10]
   5  attn_dkv_kernel (FAST) scales dK by scale_log2 instead of scale                         (test_case 4, dq4 child 1)        [9]
  20  attn_dkv_reduce_kernel skips the last split of dV                                       (test_case 17, generic child 3)   [19]
   2  frame_of drops the + 0.5f                                                               (test_case[mask_2x41-*])          [0]
The last mutant survived the table as first written ((T, HW) = (3, 49), (4, 64), (5, 1), (1, 40): x fl(1 / HW) floors right for every
token of those); mask_2x41 is the case it added (float(41) fl(1 / 41) < 1).  The one-pass mutant is seen at fused_ragged only: at
fused_tiny_kv one query row of 1030 moves a dK / dV element by less than the 16-bit rounding of the other 1029.  The old whole-tensor
tests see eight of the ten at these gross sizes; they do not see the forward FAST rescale or frame_of, nor LSE / delta as such.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected everywhere, run only on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import lib as L          # noqa: E402
import attention_core_reference as AR  # noqa: E402
import attention_raw as R              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")

# Measured bars: about 4x the worst `need` seen on MI355X over every in-process case, the three children and both libraries
# (the measured worst in the comment), never above the a priori bound of its mode.
CONSTS = {
    ("LSE", "f32"): 10.0,     # C_L: 2.44 (peaked)
    ("LSE", "h16"): 4.5,      # C_L: 1.05 (bf16, whole_fast), 1.10 (fp16, whole_fast subnormal)
    ("probs", "f32"): 8.0,    # C_P: 2.04 (mask_3x49 hd 192), 1.62 (probs_cap)
    ("probs", "h16"): 6.5,    # C_P: 1.02 (bf16, mask_3x49), 1.57 (fp16, mask_3x49)
    ("O", "f32"): 9.0,        # 2.23 (peaked)
    ("O", "h16"): 3.3,        # 0.82 (bf16, peaked), 0.40 (fp16, fused_ragged)
    ("dQ", "f32"): 1.2,       # 0.285 (peaked)
    ("dQ", "h16"): 0.65,      # 0.158 (bf16, fused_single_split), 0.085 (fp16, mask_3x49)
    ("dK", "f32"): 0.7,       # 0.177 (peaked)
    ("dK", "h16"): 0.5,       # 0.131 (bf16, peaked), 0.066 (fp16, mask_3x49 subnormal)
    ("dV", "f32"): 7.0,       # 1.76 (peaked)
    ("dV", "h16"): 3.0,       # 0.72 (bf16, mask_5x1), 0.41 (fp16, mask_3x49)
}
NK_MAX, HD_MAX = 512, 192              # the largest key count of any fwd / bwd case (staircase) and the larger head_dim


def _hold(res):
    """Print the figures, then assert every flag and bar."""
    print("\n" + R.summary(res))
    bad = R.violations(res, CONSTS)
    assert not bad, bad


def test_constants_respect_the_a_priori_bounds():
    """16-bit: C <= 4 + 2^-16 (Nk_max + hd) (1 + max A_z); fp32: C <= Nk_max + 2 hd + 16.  A measured value that needs more is a
    finding in the kernel, not a bar."""
    az = max(float(AR.reference(n, hd, R.store_key(dk))["A_z"].max()) for n, hd, dk in AR.runs(list(AR.CASES)))
    for (out, mode), c in CONSTS.items():
        if out in ("O", "dQ", "dK", "dV"):
            assert 0 < c <= (NK_MAX + 2 * HD_MAX + 16 if mode == "f32" else 4 + 2.0 ** -16 * (NK_MAX + HD_MAX) * (1 + az)), (out, mode, c, az)


# ------------------------------------------------------------------------------------------------------------ the case table
_RUNS = AR.runs(AR.IN_PROCESS)


@pytest.mark.parametrize("name,hd,dk", _RUNS, ids=[f"{n}-hd{hd}-{dk}" for n, hd, dk in _RUNS])
def test_case(name, hd, dk):
    """fwd, bwd and (masked cases) probs of one row of the case table: every element of every output against float64."""
    res, _ = R.run_case(name, hd, dk, DEV)
    _hold(res)


def test_probs_second_grid_stride_trip():
    """(1, 2, 1024, 600): 1,228,800 probabilities > 4096 x 256 threads, the last 180,224 in a second trip of the grid-stride loop."""
    assert 1228800 - 4096 * 256 == 180224
    _hold(R.run_probs_cap(DEV))


@pytest.mark.parametrize("dk", ["f32", "h16"])
def test_noop_mask_is_bit_identical(dk):
    """T = 1: every token is in frame 0, the mask kills nothing -- O, LSE, dQ, dK, dV equal the unmasked call bit for bit."""
    (rm, pm), (ru, pu) = R.run_case("mask_1x40", 96, dk, DEV), R.run_case("nomask_41", 96, dk, DEV)
    assert rm["plan"]["dkv"] == ru["plan"]["dkv"] and rm["plan"]["dq"] == ru["plan"]["dq"]
    for a, b in zip(pm.raw_fwd + pm.raw_bwd, pu.raw_fwd + pu.raw_bwd):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["ragged_both", "whole_fast", "fused_ragged"])
def test_backward_is_deterministic(name):
    """Two calls into fresh buffers: dQ, dK and dV bit-identical (the reduce sums the splits in a fixed order)."""
    pr = R.Problem(AR.reference(name, 96, R.store_key("h16")), DEV)
    assert pr.plan()["nsplit"] > 1
    pr.bwd()
    first = pr.raw_bwd
    pr.bwd()
    assert torch.equal(first[0], pr.raw_bwd[0]) and torch.equal(first[1], pr.raw_bwd[1])


def test_workspace_is_what_the_plan_implies():
    """csts_attn_bwd_workspace == 2 nsplit B H Nk hd 4 bytes, or 16, for every run of the table (no launch)."""
    lib = L.load()
    for name, hd, dk in AR.runs(list(AR.CASES)):
        B, H, Nq, Nk, _, _, mask, _ = AR.CASES[name]
        a = L.AttnArgs()
        a.dtype, a.B, a.H, a.Nq, a.Nk, a.head_dim = (L.F32 if dk == "f32" else L.BF16), B, H, Nq, Nk, hd
        if mask is not None:
            a.mask_mode, (a.mask_T, a.mask_HW) = L.MASK_SPATIAL, mask
        p = AR.plan(B, H, Nq, Nk, hd, dk == "h16", mask is not None, AR.env_of())
        assert lib.csts_attn_bwd_workspace(C.byref(a)) == p["ws"] == (2 * p["nsplit"] * B * H * Nk * hd * 4 if p["nsplit"] > 1 else 16), (name, hd, dk)


# ------------------------------------------------------------------------------------------------------------ refusals
def _refusals(name, dk, muts, check_ws):
    """Every mutation of the arguments is refused by fwd, bwd and probs (where it applies) with nothing written; the untouched
    arguments are then accepted with the same operands."""
    lib, s = L.load(), R.stream()
    pr = R.Problem(AR.reference(name, 96, R.store_key(dk)), DEV)
    o = pr.bwd_operands()
    KVf, Of, Lf = pr.kv(pr.ref["v"]), pr.dense(), pr.stat()
    P = R.f32_region(pr.B * pr.H * pr.Nq * pr.Nk, DEV).arm()
    outs = [o["dQ"], o["dKV"], o["delta"], o["ws"], Of, Lf, P]

    def afwd():
        return pr.args(KVf, Of, Lf)

    def abwd():
        return pr.args(o["KV"], o["O"], o["LSE"], o["dO"], o["delta"], o["dQ"], o["dKV"])

    def calls(mut, which="fbp", ws=None, wsz=None, probs=True):
        rc = {}
        if "f" in which:
            a = afwd(); mut(a); rc["fwd"] = lib.csts_attn_fwd(C.byref(a), s)                                      # noqa: E702
        if "b" in which:
            a = abwd(); mut(a)                                                                                      # noqa: E702
            rc["bwd"] = lib.csts_attn_bwd(C.byref(a), o["ws"].ptr() if ws is None else ws[0], o["wsz"] if wsz is None else wsz, s)
        if "p" in which:
            a = abwd(); mut(a); rc["probs"] = lib.csts_attn_probs(C.byref(a), P.ptr() if probs else None, s)       # noqa: E702
        return rc

    for what, (mut, which) in muts.items():
        rc = calls(mut, which)
        assert rc and all(v != 0 for v in rc.values()), (what, rc)
    assert all(v != 0 for v in calls(lambda a: None, "p", probs=False).values()), "null probs"
    if check_ws:
        assert o["wsz"] > 16
        assert calls(lambda a: None, "b", wsz=o["wsz"] - 1)["bwd"] != 0, "workspace one byte short"
        assert calls(lambda a: None, "b", ws=(None,))["bwd"] != 0, "null workspace"
    torch.cuda.synchronize()
    for r in outs:                                                     # nothing was launched: pre-fill and guards as armed
        assert r.guards_ok() and R.prefilled(r)
    rc = calls(lambda a: None)
    assert all(v == 0 for v in rc.values()), (rc, lib.csts_last_error())
    torch.cuda.synchronize()
    assert Of.finite() and Lf.finite() and o["dQ"].finite() and o["dKV"].finite() and P.finite() and all(r.guards_ok() for r in outs)


def _m(**kw):
    def mut(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return mut


def _shift(field, by):
    def mut(a):
        setattr(a, field, getattr(a, field) + by)
    return mut


def _stride(field, by):
    def mut(a):
        getattr(a, field)[1] += by
    return mut


_COMMON = {
    "head_dim 64": (_m(head_dim=64), "fbp"), "bad dtype": (_m(dtype=7), "fbp"), "Q off by 8 bytes": (_shift("Q", 8), "fbp"),
    "K off by 8 bytes": (_shift("K", 8), "fbp"), "dQ off by 8 bytes": (_shift("dQ", 8), "b"), "O off by 8 bytes": (_shift("O", 8), "f"),
    "null O": (_m(O=None), "fb"), "null LSE": (_m(LSE=None), "fbp"), "null dQ": (_m(dQ=None), "b"), "null dK": (_m(dK=None), "b"),
    "null dV": (_m(dV=None), "b"), "null delta": (_m(delta=None), "b"), "null dO": (_m(dO=None), "b"), "B 0": (_m(B=0), "fbp"),
}


@pytest.mark.parametrize("name,dk", [("ragged_both", "h16"), ("fused_ragged", "h16"), ("ragged_both", "f32")])
def test_refusals_launch_nothing(name, dk):
    """Bad head_dim / dtype / base / stride / null operands and a workspace one byte short, on a two-kernel shape and a one-pass
    shape: non-zero return, every output still pre-filled.  16-bit token strides must be multiples of 8 elements, fp32 of 4.
    (Before csts_attn_bwd planned its splits ahead of the first launch, the two-kernel shapes failed here: dQ and delta were
    written by a call that then returned "workspace too small".)"""
    step = 2 if dk == "f32" else 4
    muts = dict(_COMMON)
    muts.update({"q token stride": (_stride("q_strides", step), "fbp"), "k token stride": (_stride("k_strides", step), "fbp"),
                 "dk token stride": (_stride("dk_strides", step), "b"), "o token stride": (_stride("o_strides", step), "fb")})
    _refusals(name, dk, muts, check_ws=True)


def test_mask_refusals_launch_nothing():
    """The spatial mask needs Nq == Nk == T HW + T and HW > 0."""
    muts = {"Nq != T HW + T": (_m(mask_T=3, mask_HW=48), "fbp"), "Nk != Nq": (_m(Nk=149), "fbp"),
            "HW 0": (_m(mask_T=150, mask_HW=0), "fbp"), "T 0": (_m(mask_T=0, mask_HW=150), "fbp")}
    _refusals("mask_3x49", "h16", muts, check_ws=False)


def test_workspace_query_refuses_without_dividing():
    """csts_attn_bwd_workspace returns 0 for a problem the calls refuse (it touches no GPU)."""
    lib = L.load()

    def ws(**kw):
        a = L.AttnArgs()
        a.dtype, a.B, a.H, a.Nq, a.Nk, a.head_dim = L.BF16, 2, 2, 300, 100, 96
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.csts_attn_bwd_workspace(C.byref(a))

    assert ws() == 2 * 2 * 4 * 100 * 96 * 4
    for kw in ({"B": 0}, {"H": 0}, {"Nq": 0}, {"Nk": 0}, {"B": -1}, {"Nk": -5}, {"head_dim": 64}, {"head_dim": 0}):
        assert ws(**kw) == 0, kw
    assert lib.csts_attn_bwd_workspace(None) == 0


# ------------------------------------------------------------------------------------------------------------ children
@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """Three child processes, one after another, each with a timeout; the first that dies ends the run (no further child starts)."""
    out = {}
    d = tmp_path_factory.mktemp("attention")
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSTS_HALF") + AR.SWITCHES}
    for mode in AR.CHILD_CASES:
        path = d / f"{mode}.json"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attention_worker.py"), mode, str(path)], cwd=ROOT,
                           env={**base, **AR.CHILD_ENV[mode]}, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (mode, p.stderr[-4000:])
        out[mode] = json.load(open(path))
    return out


def _child_ids(mode, variants=("",)):
    return [f"{n}{v}-hd{hd}" for n, hd, _ in AR.runs(AR.CHILD_CASES[mode], half_only=True) for v in variants]


@pytest.mark.parametrize("case", _child_ids("generic"))
def test_generic_kernels_on_fast_shapes(children, case):
    """All four switches 0: the generic forward / dQ and the SLOW dK/dV at whole tiles, the two-kernel backward (which writes delta)
    on the short-kv shapes of the one-pass kernel.  Same bars."""
    res = children["generic"][case]
    assert children["generic"]["half_kind"] == 0 and res["plan"]["path"] == "two-kernel"
    assert (res["plan"]["fwd"], res["plan"]["dq"], res["plan"]["dkv"]) == ("attn_fwd_kernel<96,false>", "attn_dq_kernel<96,false>", "attn_dkv_kernel<96,false,true>")
    _hold(res)


@pytest.mark.parametrize("case", _child_ids("dq4"))
def test_dq_fast_128_key_tiles(children, case):
    """CSTS_ATTN_DQ_FAST=4: attn_dq_fast_kernel<4> on two and three 128-key tiles, the latter with a 72-row last query tile."""
    res = children["dq4"][case]
    assert res["plan"]["dq"] == "attn_dq_fast_kernel<4>"
    _hold(res)


@pytest.mark.parametrize("case", _child_ids("fp16", AR.VARIANTS))
def test_fp16_library(children, case):
    """libcsts_hip_f16.so: ordinary values, V (forward) / dO (backward) near the top of the fp16 range, channels of q / k / v in its
    subnormal range.  fp16 outputs add 2^-25 to their bar."""
    assert children["fp16"]["half_kind"] == 1
    res = children["fp16"][case]
    assert res["store"] == "fp16"
    _hold(res)
