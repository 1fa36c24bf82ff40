"""Child process of tests/test_gpu_layernorm.py: the raw LayerNorm checks of tests/layernorm_raw.py on libcsts_hip_f16.so (IEEE half),
in a process of its own because one process runs one 16-bit type.  The small-instantiation table of every C with 16-bit operands,
the csts_layernorm_fwd_add and csts_layernorm_bwd_ex cases, and two value sets only fp16 has: |x| near the top of its range
(3e4 (1 + 0.1 randn)) and x inside its subnormal range (2e-5 randn).
Writes {case: [results]} as JSON to argv[1]; the parent applies the bars."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from csts_amd import lib as L          # noqa: E402

L.set_half("fp16")
import layernorm_raw as R              # noqa: E402

DEV = torch.device("cuda:0")
EDGE_C = (8, 96, 100, 264, 767, 768)


def main(out_path):
    lib = L.load()
    H = L.half_dtype()
    assert H == torch.float16 and lib.csts_half_kind() == 1
    F = torch.float32
    out = {"half_kind": int(lib.csts_half_kind())}
    pairs = [(H, H), (F, H), (H, F)]
    for C in R.VEC_C + R.SCALAR_C:
        out[f"small_fwd_{C}"] = R.small_fwd(C, DEV, pairs)
        out[f"small_bwd_{C}"] = R.small_bwd(C, DEV, pairs)
    out["fwd_add"] = R.fwd_add_cases(DEV, H)
    for C in (96, 100):
        out[f"bwd_ex_{C}"] = R.bwd_ex_cases(DEV, H, C)
    for kind in ("big", "subnormal"):
        res = []
        for C in EDGE_C:
            res += R.run_fwd(33, C, H, H, DEV, kind=kind, seed=C) + R.run_fwd(33, C, H, F, DEV, kind=kind, seed=C + 1)
            res += R.run_bwd(33, C, H, H, DEV, kind=kind, seed=C + 2, copy="plain") + R.run_bwd(33, C, F, H, DEV, kind=kind, seed=C + 3)
        res += R.run_fwd(35, 96, H, H, DEV, kind=kind, seed=7, add="plain")
        out[kind] = res
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1])
