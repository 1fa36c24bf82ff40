"""Child process of tests/test_gpu_stencil.py: the raw stencil checks of tests/stencil_raw.py in a process of its own, because
what it varies is fixed per process -- csts_pool_ln_fwd reads CSTS_POOLLN_CPL12 once, and one process runs one 16-bit type.
  argv[1] = "cpl0": the parent set CSTS_POOLLN_CPL12=0 -- head dims 96 and 192 on 8 channels per lane, pool_ln_fwd_kernel<16 / 32, 8, ...>;
            "cpl2": CSTS_POOLLN_CPL12=2 -- the ALL27 form of the 12-channel kernel (16-bit operands only; fp32 stays on nine taps);
            "fp16": libcsts_hip_f16.so (IEEE half) -- the ragged table and the stride-(., 2, 2) block cases with ordinary values,
                    values near the top of the fp16 range and channels in its subnormal range.
Writes {case: {"conv": [results], "wgrad": [results]}} as JSON to argv[2]; the parent applies the bars."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from csts_amd import lib as L          # noqa: E402

MODE = sys.argv[1]
if MODE == "fp16":
    L.set_half("fp16")
import stencil_raw as R                # noqa: E402

DEV = torch.device("cuda:0")


def main(out_path):
    lib = L.load()
    H = L.half_dtype()
    out = {"half_kind": int(lib.csts_half_kind()), "cpl12": os.environ.get("CSTS_POOLLN_CPL12", "")}
    if MODE in ("cpl0", "cpl2"):
        assert out["cpl12"] == MODE[3] and H == torch.bfloat16
        for HD in (96, 192):
            for dt, tag in ((torch.float32, "f32"), (H, "h16")):
                out[f"pool_hd{HD}_{tag}"] = {"conv": R.pool_cases(dt, DEV, HD), "wgrad": []}
    else:
        assert H == torch.float16 and out["half_kind"] == 1
        for sfx, kw in (("", {}), ("_big", {"big": True}), ("_subnormal", {"subnormal": True})):
            for i in range(len(R.RAGGED)):
                conv, wg = R.ragged_all(H, DEV, i, **kw)
                out[f"ragged{i}{sfx}"] = {"conv": conv, "wgrad": wg}
            for i in range(len(R.S22)):
                out[f"s22_{i}{sfx}"] = {"conv": R.s22_all(H, DEV, i, **kw), "wgrad": []}
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[2])
