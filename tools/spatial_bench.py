"""Time of the on-device spatial sampling (inputs.spatial_sampling: csts_spatial_params + csts_spatial_sample) per batch against
the torch composition on the GPU (normalise, F.interpolate bilinear, slice, flip; one clip at a time, as each clip has its own
size), on the same clips and params, with the achieved rate against a byte model: output writes plus the source bytes the
crop touches (the distinct source rows the output rows read, times the span of columns the crop reads, 3 bytes a pixel).
Prints one JSON line per shape ("Spatial sampling").

    python tools/spatial_bench.py [--iters 50] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd import inputs                     # noqa: E402

DEV = torch.device("cuda:0")
MEAN, STD = (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
SHAPES = [  # name, B, T, H, W, S, jitter min, jitter max
    ("ego4d_1088x1080", 4, 16, 1088, 1080, 256, 256, 320),
    ("256sq_jitter288", 4, 16, 256, 256, 256, 288, 288),
]


def touched_bytes(params, T, H, W, S):
    """Source bytes one pass reads at least once (fp32 index arithmetic of the kernel)."""
    total = 0
    for nh, nw, y0, x0, _ in params.tolist():
        sy, sx = np.float32(H) / np.float32(nh), np.float32(W) / np.float32(nw)
        ys = np.maximum((np.arange(y0, y0 + S, dtype=np.float32) + np.float32(0.5)) * sy - np.float32(0.5), np.float32(0))
        ya = np.minimum(ys.astype(np.int64), H - 1)
        rows = np.unique(np.concatenate([ya, np.minimum(ya + 1, H - 1)]))
        xs = np.maximum((np.array([x0, x0 + S - 1], dtype=np.float32) + np.float32(0.5)) * sx - np.float32(0.5), np.float32(0))
        xlo, xhi = min(int(xs[0]), W - 1), min(int(xs[1]) + 1, W - 1)
        total += len(rows) * (xhi - xlo + 1) * 3 * T
    return total


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / iters        # us per call


def torch_composition(frames, params, S):
    m = torch.tensor(MEAN, device=DEV).view(3, 1, 1, 1)
    s = torch.tensor(STD, device=DEV).view(3, 1, 1, 1)
    out = []
    for b, (nh, nw, y0, x0, flip) in enumerate(params):
        v = (frames[b].permute(3, 0, 1, 2).float() / 255.0 - m) / s                       # 3 T H W
        v = F.interpolate(v.permute(1, 0, 2, 3), size=(nh, nw), mode="bilinear", align_corners=False)
        v = v[..., y0:y0 + S, x0:x0 + S]
        out.append(v.flip(-1) if flip else v)
    return torch.stack(out).permute(0, 2, 1, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spatial_bench.py measures on the GPU; none is visible")
    lines = []
    for name, B, T, H, W, S, mn, mx in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(0)
        frames = torch.randint(0, 256, (B, T, H, W, 3), generator=g, device=DEV, dtype=torch.uint8)
        lab = torch.rand(B, T, 3, generator=g, device=DEV)
        torch.manual_seed(0)
        video, _, params = inputs.spatial_sampling(frames, lab, S, train=True, min_scale=mn, max_scale=mx, return_params=True)
        plist = [tuple(int(v) for v in p) for p in params.cpu()]
        ref = torch_composition(frames, plist, S)
        err = float((video - ref).abs().max())
        t_fused = timed(lambda: inputs.spatial_sampling(frames, lab, S, train=True, min_scale=mn, max_scale=mx), args.iters)
        t_sample = timed(lambda: inputs.spatial_sample(frames, params, S), args.iters)
        t_torch = timed(lambda: torch_composition(frames, plist, S), max(5, args.iters // 5))
        out_bytes = B * 3 * T * S * S * 4
        src_bytes = touched_bytes(params.cpu(), T, H, W, S)
        rec = {"shape": name, "B": B, "T": T, "H": H, "W": W, "S": S, "jitter": [mn, mx], "params": plist,
               "fused_us": round(t_fused, 1), "sample_kernel_us": round(t_sample, 1), "torch_us": round(t_torch, 1),
               "speedup_vs_torch": round(t_torch / t_fused, 1), "model_MB": round((out_bytes + src_bytes) / 1e6, 2),
               "sample_GBps": round((out_bytes + src_bytes) / (t_sample * 1e-6) / 1e9, 1), "max_abs_vs_torch": err}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
