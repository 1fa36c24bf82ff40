"""SHA-256 of every output tensor of the depthwise stencil entries on the shared problem sets of tests/stencil_raw.py: the check
that a restructuring of csts_amd/csrc/stencil.hip is bit-identical (no floating-point sum may be reordered; the build has
-ffp-contract=off).  One line per output region: case, output, digest of the region's bytes.  Run it once per library
(CSTS_HIP_LIB / CSTS_HIP_LIB_F16 name the build) and per configuration, each in a process of its own, and diff the listings:
    python tools/stencil_digest.py [bf16 | fp16] > listing         (CSTS_POOLLN_CPL12=0 | 2 in the environment for those forms)
Problem sets: the ragged table through strided, transposed, pool + LayerNorm and the weight gradient; the 2 x 2-block transposed
cases; pool_cases and pool_tiny at every head dim of POOL_HEADS (conv_out, y, mean, rstd); the weight-gradient entries in all
four modes (workspace and dweight)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from csts_amd import lib as L          # noqa: E402

HALF = sys.argv[1] if len(sys.argv) > 1 else "bf16"
L.set_half(HALF)
import stencil_raw as R                # noqa: E402

DEV = torch.device("cuda:0")


def digest(case, run):
    R.OUTPUTS = []
    run()
    for name, reg in R.OUTPUTS:
        data = reg._strided(reg.ibuf).contiguous().cpu().numpy().tobytes()
        print(f"{case} | {name} {tuple(reg.view().shape)} | {hashlib.sha256(data).hexdigest()}")
    R.OUTPUTS = None


def main():
    lib = L.load()
    H = L.half_dtype()
    print(f"# half_kind {int(lib.csts_half_kind())} CSTS_POOLLN_CPL12={os.environ.get('CSTS_POOLLN_CPL12', '')}")
    for dt, tag in ((torch.float32, "f32"), (H, "h16")):
        for i in range(len(R.RAGGED)):
            digest(f"ragged{i} {tag}", lambda: R.ragged_all(dt, DEV, i))
        for HD in R.POOL_HEADS:
            digest(f"pool_cases hd{HD} {tag}", lambda: R.pool_cases(dt, DEV, HD))
            digest(f"pool_tiny hd{HD} {tag}", lambda: R.pool_tiny(dt, DEV, HD))
        specs = R.wgrad_specs()
        for mode in ("dweight", "null"):
            digest(f"wgrad {mode} {tag}", lambda: R.run_wgrad([R.WgradProblem(s, dt, DEV) for s in specs], mode, DEV))
        digest(f"wgrad two {tag}",
               lambda: R.run_wgrad([(R.WgradProblem(s, dt, DEV, seed=4), R.WgradProblem(s, dt, DEV, seed=14)) for s in specs], "two", DEV))
        digest(f"wgrad grouped {tag}", lambda: R.run_wgrad_grouped([R.WgradProblem(s, dt, DEV) for s in specs], DEV))
    for i in range(len(R.S22)):
        digest(f"s22_{i} h16", lambda: R.s22_all(H, DEV, i))


if __name__ == "__main__":
    main()
