#!/usr/bin/env python3
"""What the fusion attention maps cost on the GPU, at the benchmark configuration (b = 4, 8 x 256^2, bf16, one GPU), three
comparisons in ONE process ("Fusion attention maps"):

  1. predict   the captured forward-only step (csts_amd.infer.GraphedEvalStep) replayed
                 plain      as predict_batch() runs it,
                 attention  as predict_batch(attention=True) runs it (csts_audio_pixel_attn on the block's qkv and lse),
                 parent     the composition that existed before: the forward with return_spatial_attn / return_temporal_attn (the
                            whole (B, heads, N, N) probability matrix), then torch slicing, F.interpolate(trilinear) to T x S x S and
                            amin / amax / rescale per frame -- captured and replayed the same way;
               the figure of merit is what each adds to `plain`.
  2. op        ops.audio_pixel_attn alone on the qkv / lse of that forward, against attention_probs + the same torch composition.
  3. render    GazePredictor.render_attention (eager calls: it uploads its params row), the ops.gaze_overlay launch behind it
               replayed from a graph, and out.copy_(frames) of the same bytes.

Rounds alternate the variants; one event pair spans `--steps` replays.  Medians and the spread over rounds go to --out.

    python tools/attention_bench.py                                # -> profiles/attention_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                  # noqa: E402
from csts_amd import lib as L                       # noqa: E402
from csts_amd import ops, train as T                # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402
from csts_amd.infer import GazePredictor, GraphedEvalStep, TEMPERATURE   # noqa: E402


def parent_maps(spatial_attn, thw, n_frames, S):
    """visualization.py:189-216 from torch ops on the full probabilities: slice, stack, upsample, per-frame min-max."""
    Tp, h, w = thw
    HW = h * w
    col = torch.stack([spatial_attn[:, :, HW * t:HW * (t + 1), Tp * HW + t] for t in range(Tp)], dim=2)
    col = col.reshape(col.shape[0], col.shape[1], Tp, h, w)
    up = torch.nn.functional.interpolate(col, size=(n_frames, S, S), mode="trilinear", align_corners=False)
    lo, hi = up.amin(dim=(-2, -1), keepdim=True), up.amax(dim=(-2, -1), keepdim=True)
    return col, (up - lo) / (hi - lo + 1e-6)


def graphed(fn, warmup):
    """fn captured into a HIP graph the way GraphedEvalStep captures its step."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ops.refill_capture_pools()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        keep = fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph, keep


def time_calls(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n              # us per call


def compare(variants, rounds, steps):
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(time_calls(fn, steps))
    return {k: {"median_us": round(statistics.median(v), 2), "round_us": [round(x, 2) for x in v],
                "round_spread_us": round(max(v) - min(v), 2)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30, help="replays between the two events of one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/attention_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", args.frames, "CSTS_AMD.COMPUTE", args.compute])
    torch.manual_seed(cfg.RNG_SEED)
    pred = GazePredictor(cfg, device=dev, graph=True)
    model = pred.model
    S = int(cfg.DATA.TEST_CROP_SIZE)
    batch = T.synthetic_batch(args.batch, args.frames, S, 2000, dev)
    video, audio = batch["video"].contiguous(), batch["audio"].contiguous()
    res = {"tool": "attention_bench", "device": torch.cuda.get_device_name(0), "batch": args.batch, "frames": args.frames,
           "compute": args.compute, "rounds": args.rounds, "replays_per_round": args.steps, "warmup": args.warmup,
           "build": build_stamp.current()}
    with torch.no_grad():
        # the inputs of the op, as the spatial fusion block holds them
        grabbed = {}
        real = ops.audio_pixel_attn

        def grab(qkv, lse, thw, heads, n_frames, crop):
            grabbed.update(qkv=qkv.clone(), lse=lse.clone(), thw=list(thw), heads=heads)
            return real(qkv, lse, thw, heads, n_frames, crop)

        ops.audio_pixel_attn = grab
        try:
            model([video], audio, return_fusion_maps=True)
        finally:
            ops.audio_pixel_attn = real
        qkv, lse, thw, heads = grabbed["qkv"], grabbed["lse"], grabbed["thw"], grabbed["heads"]
        B, N, C3 = qkv.shape
        res["spatial_fusion"] = {"qkv": list(qkv.shape), "dtype": str(qkv.dtype), "grid": thw, "heads": heads,
                                 "dots_new": heads * thw[0] * thw[1] * thw[2] * B, "dots_parent": heads * N * N * B}

        # ---- 1. the predict step
        def parent_step():
            logits, sp, tp = model([video], audio, return_spatial_attn=True, return_temporal_attn=True)
            out = ops.gaze_decode(logits, TEMPERATURE)
            out["column"], out["maps"] = parent_maps(sp, thw, args.frames, S)
            out["temporal"] = tp.mean(dim=1)
            return out

        plain = GraphedEvalStep(cfg, model, {"video": video, "audio": audio})
        attn = GraphedEvalStep(cfg, model, {"video": video, "audio": audio}, attention=True)
        g_parent, out_parent = graphed(parent_step, args.warmup)
        a = attn.run()
        p = plain.run()
        torch.cuda.synchronize()
        rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
        res["outputs"] = {"heatmaps_bit_equal_with_and_without_attention": bool(torch.equal(a["preds"], p["preds"])),
                          "column_new_vs_parent_rel_l2": rel(a["audio_attention"], out_parent["column"]),
                          "temporal_new_vs_parent_rel_l2": rel(a["temporal_attention"], out_parent["temporal"])}
        r1 = compare({"plain": plain.graph.replay, "attention": attn.graph.replay, "parent": g_parent.replay}, args.rounds, args.steps)
        added_new = r1["attention"]["median_us"] - r1["plain"]["median_us"]
        added_parent = r1["parent"]["median_us"] - r1["plain"]["median_us"]
        r1["attention_adds_us"] = round(added_new, 2)
        r1["parent_adds_us"] = round(added_parent, 2)
        r1["parent_adds_over_attention_adds"] = round(added_parent / added_new, 2) if added_new > 0 else None
        r1["attention_adds_less_than_parent"] = bool(added_new < added_parent)
        res["predict"] = r1
        print("predict: " + json.dumps({k: (v["median_us"] if isinstance(v, dict) else v) for k, v in r1.items()}), flush=True)

        # ---- 2. the op alone
        def op_new():
            return ops.audio_pixel_attn(qkv, lse, thw, heads, args.frames, S)

        def op_parent():
            probs = ops.attention_probs(qkv, B, N, C3 // 3, heads, lse, L.MASK_SPATIAL, thw[0], thw[1] * thw[2])
            return parent_maps(probs, thw, args.frames, S)

        g_new, o_new = graphed(op_new, args.warmup)
        g_old, o_old = graphed(op_parent, args.warmup)
        r2 = compare({"audio_pixel_attn": g_new.replay, "parent": g_old.replay}, args.rounds, args.steps)
        r2["parent_over_new"] = round(r2["parent"]["median_us"] / r2["audio_pixel_attn"]["median_us"], 2)
        r2["column_rel_l2"] = rel(o_new["column"], o_old[0])
        r2["bytes_written_new"] = sum(v.numel() * 4 for v in o_new.values())
        r2["bytes_written_parent_probs"] = B * heads * N * N * 4
        res["op"] = r2
        print("op: " + json.dumps({k: (v["median_us"] if isinstance(v, dict) else v) for k, v in r2.items()}), flush=True)

        # ---- 3. drawing
        result = pred.predict_batch(batch, attention=True)
        res["render"] = {}
        for H, W in ((S, S), (1080, 1440)):
            frames = torch.randint(0, 256, (args.batch, args.frames, H, W, 3), device=dev, dtype=torch.uint8,
                                   generator=torch.Generator(device=dev).manual_seed(H))
            out_r, out_k, out_c = torch.empty_like(frames), torch.empty_like(frames), torch.empty_like(frames)
            n = args.batch * args.frames
            params = torch.tensor(pred._video_params_row(H, W), dtype=torch.int32, device=dev)
            maps = result["attention_maps"][:, -1].reshape(n, thw[1], thw[2]).contiguous()
            g_k, _ = graphed(lambda: ops.gaze_overlay(frames.view(n, H, W, 3), maps, params, S, out=out_k.view(n, H, W, 3)), args.warmup)
            g_c, _ = graphed(lambda: out_c.copy_(frames), args.warmup)
            for _ in range(args.warmup):
                pred.render_attention(frames, result, out=out_r)
            r3 = compare({"render_attention_eager": lambda: pred.render_attention(frames, result, out=out_r),
                          "gaze_overlay_graph": g_k.replay, "copy_graph": g_c.replay}, args.rounds, args.steps)
            r3["same_bytes_as_gaze_overlay"] = bool(torch.equal(out_r, out_k))
            r3["bytes_in_plus_out"] = 6 * n * H * W
            r3["overlay_over_copy"] = round(r3["gaze_overlay_graph"]["median_us"] / r3["copy_graph"]["median_us"], 2)
            res["render"][f"{H}x{W}"] = r3
            print(f"render {H}x{W}: " + json.dumps({k: (v["median_us"] if isinstance(v, dict) else v) for k, v in r3.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
