"""Child process of tests/test_gpu_attention_core.py: the raw attention checks of tests/attention_raw.py in a process of its own,
because what it varies is fixed per process -- the host code reads its four switches once, and one process runs one 16-bit type.
  argv[1] = "generic": the parent set CSTS_ATTN_FWD_FAST, _DQ_FAST, _DKV_FAST and _FUSED_BWD to 0 -- the generic forward / dQ and the
                       SLOW dK/dV at whole tiles, the two-kernel backward on short-kv shapes;
            "dq4":     CSTS_ATTN_DQ_FAST=4 -- attn_dq_fast_kernel<4> (128-key tiles);
            "fp16":    libcsts_hip_f16.so (IEEE half) -- ordinary values, values near the top of the fp16 range, channels of
                       q / k / v in its subnormal range.
The cases are attention_core_reference.CHILD_CASES[mode], 16-bit runs only.  Writes {"<case><variant>-hd<hd>": result} as JSON to
argv[2]; the parent applies the bars."""
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
import attention_core_reference as AR  # noqa: E402
import attention_raw as R              # noqa: E402

DEV = torch.device("cuda:0")


def main(out_path):
    lib = L.load()
    out = {"half_kind": int(lib.csts_half_kind()), "env": {k: os.environ.get(k, "") for k in AR.SWITCHES}}
    assert out["half_kind"] == (1 if MODE == "fp16" else 0)
    for k, v in AR.CHILD_ENV[MODE].items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    for name, hd, dk in AR.runs(AR.CHILD_CASES[MODE], half_only=True):
        for variant in (AR.VARIANTS if MODE == "fp16" else ("",)):
            res, _ = R.run_case(name, hd, dk, DEV, variant)
            print(R.summary(res), flush=True)
            out[f"{name}{variant}-hd{hd}"] = res
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[2])
