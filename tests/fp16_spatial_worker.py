"""Child process of tests/test_gpu_spatial.py: spatial_sampling in the fp16 kernel library (libcsts_hip_f16.so; one 16-bit type
per process, so this cannot share pytest's process with the bf16 library).  Same seeded inputs and key as the parent; saves
{video, labels, params} to argv[1]."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd import lib                         # noqa: E402

lib.set_half("fp16")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_spatial import fp16_parity_case    # noqa: E402


if __name__ == "__main__":
    assert lib.load().csts_half_kind() == 1
    torch.save(fp16_parity_case(), sys.argv[1])
