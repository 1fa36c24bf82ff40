"""SHA-256 of every output tensor of the LayerNorm entries on the shared problem sets of tests/layernorm_raw.py: the check that a
restructuring of csts_amd/csrc/norm.hip is bit-identical (no floating-point sum may be reordered; the build has -ffp-contract=off).
One line per output region: case | output, shape, digest of the region's bytes -- y, mean, rstd, sum_out; dx, the 16-bit copy, the
partial rows of the workspace and dgamma | dbeta.  Run it once per library (CSTS_HIP_LIB / CSTS_HIP_LIB_F16 name the build), each
in a process of its own, and diff the listings:
    python tools/ln_digest.py [bf16 | fp16] > listing         (without an argument: CSTS_HALF)
Problem sets: the small table of every VEC_C and SCALAR_C, forward and backward; one operand off its alignment at the model widths;
the grid-stride trips; csts_layernorm_fwd_add; csts_layernorm_bwd_ex; the deferred second stage beside the immediate one;
csts_layernorm_bwd2."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from csts_amd import lib as L          # noqa: E402

HALF = sys.argv[1] if len(sys.argv) > 1 else L.HALF
L.set_half(HALF)
import layernorm_raw as R              # noqa: E402

DEV = torch.device("cuda:0")
F = torch.float32


def digest(case, run):
    R.OUTPUTS = []
    run()
    for name, buf in R.OUTPUTS:
        data = buf.view().contiguous().view(torch.uint8).cpu().numpy().tobytes()
        print(f"{case} | {name} ({buf.n}) | {hashlib.sha256(data).hexdigest()}")
    R.OUTPUTS = None


def main():
    lib = L.load()
    H = L.half_dtype()
    print(f"# half_kind {int(lib.csts_half_kind())}")
    pairs = [(F, F), (F, H), (H, F), (H, H)]
    for C in R.VEC_C + R.SCALAR_C:
        digest(f"small_fwd {C}", lambda: R.small_fwd(C, DEV, pairs))
        digest(f"small_bwd {C}", lambda: R.small_bwd(C, DEV, pairs))
    for C in R.MISALIGNED_C:
        digest(f"misaligned {C}", lambda: R.misaligned_cases(DEV, H, C))
    for C, rows, xdt, ydt in R.fwd_trips(H):
        digest("fwd_trips", lambda: R.run_fwd(rows, C, xdt, ydt, DEV, kind="offset", seed=C))
    for C, rows, dydt, xdt, _ in R.bwd_trips(H):
        digest("bwd_trips", lambda: R.run_bwd(rows, C, dydt, xdt, DEV, kind="offset", seed=C))
    digest("fwd_add", lambda: R.fwd_add_cases(DEV, H))
    for C in (96, 100, 384):
        digest(f"bwd_ex {C}", lambda: R.bwd_ex_cases(DEV, H, C))
    for C, rows in R.DEFERRED:
        for deferred in (False, True):
            digest("deferred", lambda: R.run_bwd(rows, C, H, F, DEV, kind="offset", seed=C, ex=True, deferred=deferred))
    for C, rows in R.BWD2:
        for dydt, xdt in R.bwd2_pairs(C, rows, H):
            digest("bwd2", lambda: R.run_bwd2(rows, C, dydt, xdt, DEV, seed=C + rows))


if __name__ == "__main__":
    main()
