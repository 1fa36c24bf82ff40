#!/usr/bin/env python3
"""Time of the gaze overlay drawn in 4:2:0 (ops.gaze_overlay_yuv, csts_gaze_overlay_yuv) on NV12 frames against what a renderer
given such frames did before it, on the same box, in the same process:
  (a) rgb_path              inputs.yuv_to_rgb into an RGB tensor + ops.gaze_overlay in place there: RGB out, 4.5 + up to 6 bytes a pixel;
  (b) rgb_path_to_nv12      (a) + inputs.rgb_to_yuv: what it takes to hand NV12 to an encoder without the new op;
  (c) gaze_overlay_yuv      the new op, out of place: 1.5 bytes in + 1.5 bytes out a pixel;
  (d) gaze_overlay_yuv_in_place   the new op with out = frames;
  (e) copy                  out.copy_(frames) of the 4:2:0 bytes: the streaming floor of (c).
16 frames of 1088 x 1080 (H x W; rows of 1080 bytes start at no multiple of 16) with a 64 x 64 map, S 256, alpha 0.4, radius 5, one
marker per frame.  Every variant is captured in a HIP graph of its own and replayed; rounds alternate the variants, one event pair
around `--steps` replays each; the medians over the rounds are reported.  Before timing, (c) is compared with the composition
where(M, rgb_to_yuv(D), frames) formed from (a), (b) and the mask drawn by ops.gaze_overlay over black frames.

    python tools/overlay_yuv_bench.py                              # -> profiles/overlay_yuv_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                  # noqa: E402
from csts_amd import inputs, ops                    # noqa: E402
from overlay_bench import graphed, time_replays     # noqa: E402


def composition(frames, encoded, mask, H, W):
    """where(M, rgb_to_yuv(D), frames) for NV12 on the device: mask bool (N, H, W) per pixel for luma, per 2 x 2 block (any) for
    the interleaved chroma rows."""
    blk = mask[:, 0::2, 0::2] | mask[:, 0::2, 1::2] | mask[:, 1::2, 0::2] | mask[:, 1::2, 1::2]
    full = torch.cat([mask, blk.repeat_interleave(2, dim=-1)], dim=1)                  # (N, H * 3 / 2, W)
    return torch.where(full, encoded, frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="replays between the two events of one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_yuv_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/overlay_yuv_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    N, H, W, S, M, alpha, radius = 16, 1088, 1080, 256, 64, 0.4, 5
    fmt = {"pixel_format": "nv12", "matrix": "bt709", "full_range": False}
    g = torch.Generator(device=dev).manual_seed(H)
    frames = torch.randint(0, 256, (N, H * 3 // 2, W), generator=g, device=dev, dtype=torch.uint8)
    p = torch.softmax(torch.randn(N, M * M, generator=g, device=dev) / 2, dim=-1)
    mn, mx = p.amin(dim=-1, keepdim=True), p.amax(dim=-1, keepdim=True)
    maps = ((p - mn) / (mx - mn + 1e-6)).reshape(N, M, M).contiguous()
    row = inputs.spatial_rule_host(np.zeros((1, 1, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()
    params = torch.tensor(row, dtype=torch.int32, device=dev)
    centers = torch.stack([torch.randint(0, W, (N,), generator=g, device=dev), torch.randint(0, H, (N,), generator=g, device=dev)],
                          dim=-1).to(torch.int32)
    kw = dict(centers=centers, alpha=alpha, radius=radius)
    rgb = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    back, out_y, out_c, work = (torch.empty_like(frames) for _ in range(4))
    work.copy_(frames)

    def rgb_path():
        inputs.yuv_to_rgb(frames, out=rgb, **fmt)
        return ops.gaze_overlay(rgb, maps, params, S, out=rgb, **kw)

    def rgb_path_to_nv12():
        return inputs.rgb_to_yuv(rgb_path(), out=back, **fmt)

    variants = {"rgb_path": rgb_path,
                "rgb_path_to_nv12": rgb_path_to_nv12,
                "gaze_overlay_yuv": lambda: ops.gaze_overlay_yuv(frames, maps, params, S, out=out_y, **kw, **fmt),
                "gaze_overlay_yuv_in_place": lambda: ops.gaze_overlay_yuv(work, maps, params, S, out=work, **kw, **fmt),
                "copy": lambda: out_c.copy_(frames)}
    # the same bytes first: the new op against the composition of the parent's path
    black = ops.gaze_overlay(torch.zeros_like(rgb), maps, params, S, centers=centers, alpha=1.0, radius=radius)
    mask = (black != 0).any(dim=-1)
    want = composition(frames, rgb_path_to_nv12(), mask, H, W)
    differing = int((variants["gaze_overlay_yuv"]() != want).sum())
    in_place_differing = int((variants["gaze_overlay_yuv_in_place"]() != want).sum())
    work.copy_(frames)
    graphs = {k: graphed(fn, args.warmup) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, gr in graphs.items():
            times[k].append(time_replays(gr, args.steps))
    pixels = N * H * W
    model = {"rgb_path": 4.5 + 6.0, "rgb_path_to_nv12": 4.5 + 6.0 + 4.5, "gaze_overlay_yuv": 3.0, "gaze_overlay_yuv_in_place": 3.0,
             "copy": 3.0}                                                               # bytes a pixel at most, the byte model
    res = {"tool": "overlay_yuv_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "replays_per_round": args.steps, "warmup": args.warmup, "build": build_stamp.current(), "frames": N, "shape": [H, W],
           "map": [M, M], "params": row, "format": fmt, "drawn_pixels": int(mask.sum()), "pixels": pixels,
           "bytes_differing_from_composition": differing, "in_place_bytes_differing_from_composition": in_place_differing}
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = {"median_us": round(med, 2), "round_us": [round(x, 2) for x in v], "round_spread_us": round(max(v) - min(v), 2),
                  "model_bytes_per_pixel": model[k], "model_gb_per_s": round(model[k] * pixels / med / 1e3, 1)}
    med = {k: res[k]["median_us"] for k in variants}
    res["rgb_path_over_yuv"] = round(med["rgb_path"] / med["gaze_overlay_yuv"], 2)
    res["rgb_path_to_nv12_over_yuv"] = round(med["rgb_path_to_nv12"] / med["gaze_overlay_yuv"], 2)
    res["rgb_path_to_nv12_over_yuv_in_place"] = round(med["rgb_path_to_nv12"] / med["gaze_overlay_yuv_in_place"], 2)
    res["yuv_over_copy"] = round(med["gaze_overlay_yuv"] / med["copy"], 2)
    res["yuv_not_slower_than_rgb_path"] = bool(med["gaze_overlay_yuv"] <= med["rgb_path"])
    res["yuv_beats_rgb_path_beyond_spread"] = bool(max(times["gaze_overlay_yuv"]) < min(times["rgb_path"]))
    print(", ".join(f"{k} {med[k]} us" for k in variants) + f"; rgb path / yuv {res['rgb_path_over_yuv']}, rgb path to nv12 / yuv "
          f"{res['rgb_path_to_nv12_over_yuv']}, yuv / copy {res['yuv_over_copy']}; bytes differing from the composition {differing} "
          f"(in place {in_place_differing})", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
