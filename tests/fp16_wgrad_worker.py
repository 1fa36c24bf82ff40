"""Child process of tests/test_gpu_wgrad.py: the raw-table checks of tests/wgrad_raw.py on the fp16 library (libcsts_hip_f16.so,
IEEE-half operands) for csts_wgrad_grouped8, csts_wgrad_grouped5 and csts_wgrad_grouped (16-bit and fp32 dY), with ordinary values,
values near the top of the fp16 range and features in the fp16 subnormal range.  One process runs one 16-bit type, so this cannot
share pytest's process with the bf16 checks.  Writes {case: [[per-output result]]} as JSON to argv[1]; the parent applies the bars."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from csts_amd import lib as L          # noqa: E402

L.set_half("fp16")
import wgrad_raw as R                  # noqa: E402

DEV = torch.device("cuda:0")
H = torch.float16


def run(kind, probs, tm, tn, pad_every, **kw):
    its = [it for p in probs for it in p.items(tm, tn, w5=(kind == "w5"))]
    if kind == "w8":
        its = R.w8_items(probs)
    table, n = R.upload(its, DEV, pad_every=pad_every)
    R.launch(kind, table, n, **kw)
    torch.cuda.synchronize()
    return [p.check() for p in probs]


def main(out_path):
    lib = L.load()
    out = {"half_kind": int(lib.csts_half_kind())}
    assert L.half_dtype() == H
    for sfx, kw in (("", {}), ("_big", {"big": True}), ("_subnormal", {"subnormal": True})):
        out["w8" + sfx] = run("w8", R.w8_problems(DEV, H, **kw), 192, 384, 7)
        out["w5" + sfx] = run("w5", R.w5_problems(DEV, H, **kw), 96, 96, 5)
    out["wg_h16"] = run("wg", R.wg_problems(DEV, H, H), 128, 128, 3, a_f32=0, rows=128)
    out["wg_h16_big"] = run("wg", R.wg_problems(DEV, H, H, big=True), 256, 128, 3, a_f32=0, rows=256)
    out["wg_f32"] = run("wg", R.wg_problems(DEV, torch.float32, H), 128, 128, 3, a_f32=1, rows=128)
    out["wg_f32_subnormal"] = run("wg", R.wg_problems(DEV, torch.float32, H, subnormal=True), 64, 128, 3, a_f32=1, rows=64)
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1])
