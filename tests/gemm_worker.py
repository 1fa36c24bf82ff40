"""Child process of tests/test_gpu_gemm.py: the raw GEMM checks of tests/gemm_raw.py in a process of its own.
  fp16    on libcsts_hip_f16.so (IEEE half; one process runs one 16-bit type): gemm_raw.fp16_cases() -- one exact and one random case
          per family, every gemm5 form, gemm4 forms 2, 4 and 5, |C| near the top of the fp16 range and C in its subnormal range.
  switch  on the bf16 library with gemm_raw.SWITCH_ENV set by the parent (the library reads its switches once per process):
          gemm_raw.switch_cases() under algo 0.
Writes {case id: result} as JSON to argv[2]; the parent applies the bars.  argv[3]: the parent's BARS as JSON."""
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
import gemm_raw as R                   # noqa: E402

DEV = torch.device("cuda:0")


def main(out_path, bars):
    lib = L.load()
    out = {"half_kind": int(lib.csts_half_kind())}
    if MODE == "fp16":
        assert L.half_dtype() == torch.float16 and out["half_kind"] == 1
        cases = R.fp16_cases()
    else:
        assert all(os.environ.get(k) == v for k, v in R.SWITCH_ENV.items())
        cases = R.switch_cases()
    for cid, _, c in cases:
        out[cid] = R.run(c, DEV, bars)
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[2], json.loads(sys.argv[3]))
