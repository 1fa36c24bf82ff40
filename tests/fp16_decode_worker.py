"""Child process of tests/test_gpu_decode.py: the gaze_decode cases in the fp16 kernel library (libcsts_hip_f16.so; one 16-bit
type per process, so this cannot share pytest's process with the bf16 library): fp32 logits and IEEE-half logits against the
float64 composition, with the bounds of the parent."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd import lib                         # noqa: E402

lib.set_half("fp16")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_decode import check_all_cases      # noqa: E402


if __name__ == "__main__":
    assert lib.load().csts_half_kind() == 1 and lib.half_dtype() == torch.float16
    assert check_all_cases((torch.float32, torch.float16))
    print("fp16 decode cases passed")
