"""The library's own attention route (csts_attn_route, csts_attn_bwd_workspace: both host-only) held to the restatement
attention_core_reference.plan().  tests/test_attention_core_reference_host.py calls mismatches() in-process for the default
environment and runs this file as a child for every other one, because what varies is fixed per process: the host code reads its
four switches once, and one process runs one 16-bit library (CSTS_HALF).  The child never touches the GPU.
  python tests/attention_route_worker.py OUT.json
writes {"env": the switches as this process read them, "half_kind", "checked", "bad": the first mismatches}."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from csts_amd import lib as L          # noqa: E402
import attention_core_reference as AR  # noqa: E402

# the sweep of test_reduce_second_trip_is_unreachable, widened so that every threshold of the plan is hit on both sides
SWEEP_BH = (1, 2, 3, 7, 64, 127, 128, 129, 256, 257)
SWEEP_NK = (1, 8, 64, 65, 127, 128, 129, 192, 1024, 16384, 16385, 1 << 17)
SWEEP_NQ = (1, 127, 255, 256, 1023, 1024, 4096, 1 << 17)


def problems():
    """(B, H, Nq, Nk, hd, h16, mask (T, HW) or None): every run of CASES, PROBS_CAP and the sweep."""
    out = []
    for name, hd, dk in AR.runs(AR.CASES):
        B, H, Nq, Nk, _, _, mask, _ = AR.CASES[name]
        out.append((B, H, Nq, Nk, hd, dk == "h16", mask))
    out.append(AR.PROBS_CAP + (False, None))
    out += [(1, BH, Nq, Nk, hd, h16, None) for h16 in (False, True) for hd in (96, 192) for BH in SWEEP_BH for Nk in SWEEP_NK
            for Nq in SWEEP_NQ]
    return out


def args_of(B, H, Nq, Nk, hd, h16, mask):
    """The fields the route reads; every operand pointer stays NULL."""
    a = L.AttnArgs()
    a.dtype, a.B, a.H, a.Nq, a.Nk, a.head_dim = (L.BF16 if h16 else L.F32), B, H, Nq, Nk, hd
    if mask is not None:
        a.mask_mode, a.mask_T, a.mask_HW = L.MASK_SPATIAL, mask[0], mask[1]
    return a


def route(lib, a):
    """(rc, [fwd, dq, dkv, reduce], nsplit, q_chunk) of csts_attn_route."""
    buf, ns, qc = C.create_string_buffer(160), C.c_int(0), C.c_int(0)
    rc = lib.csts_attn_route(C.byref(a) if a is not None else None, buf, 160, C.byref(ns), C.byref(qc))
    return rc, buf.value.decode().split(";"), ns.value, qc.value


def mismatches(lib, env):
    """(problems checked, [(problem, library, restatement)]) under the switches `env` (AR.env_of of the process's environment)."""
    bad = []
    probs = problems()
    for pr in probs:
        B, H, Nq, Nk, hd, h16, mask = pr
        p = AR.plan(B, H, Nq, Nk, hd, h16, mask is not None, env)
        want = ([p["fwd"], p["dq"] or "", p["dkv"], "attn_dkv_reduce_kernel" if p["reduce"] else ""], p["nsplit"], p["q_chunk"], p["ws"])
        a = args_of(*pr)
        rc, names, ns, qc = route(lib, a)
        if rc == 0 and names[2] == "attn_bwd_fused_kernel" and ns == 1:
            names[2] += "/direct"                                     # the direct-store branch the restatement names apart
        got = (names, ns, qc, lib.csts_attn_bwd_workspace(C.byref(a)))
        if rc != 0 or got != want:
            bad.append((pr, (rc,) + got, want))
    return len(probs), bad


def main(out_path):
    L.set_half(L.HALF)                                                # CSTS_HALF=fp16: the IEEE-half build
    lib = L.load()
    env = AR.env_of()
    n, bad = mismatches(lib, env)
    with open(out_path, "w") as f:
        json.dump({"env": env, "half_kind": int(lib.csts_half_kind()), "checked": n, "n_bad": len(bad), "bad": bad[:5]}, f)


if __name__ == "__main__":
    main(sys.argv[1])
