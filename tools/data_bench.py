"""Batch assembly from recorded clips, measured in ONE process ("Recorded clips"):

  (a) loader       the device half of datasets.ClipLoader.batch (batch_params, batch_sample, audio_gather, label gather,
                   gaze_heatmaps) captured in one HIP graph and replayed: b 4, T 8, source 256 x 341, S 256, train mode;
  (b) composition  the same batch from the single-recording ops: per clip spatial_params + clip_sample + audio_windows_at +
                   gaze_heatmaps, then cat -- eagerly and as a captured graph;
  (c) bench        `python bench.py --gpus 1` in child processes, alternating this tree and (with --parent-tree DIR, a built tree
                   of the parent commit) the parent: clips/s per run, their medians and the run-to-run spread.

(a) and (b) are alternated over several rounds after a warm-up; a round times `--steps` calls between two device events.  Writes the
JSON (with the build stamp) to --out and prints it on one line.

    python tools/data_bench.py [--parent-tree DIR] [--bench-runs 3]         # -> profiles/data_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                   # noqa: E402
from make_toy_dataset import write_dataset           # noqa: E402
from video_bench import alternate                    # noqa: E402
from csts_amd import datasets as D, inputs, lib      # noqa: E402
from csts_amd.config import load_yaml                # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def bench_runs(trees, runs, steps, warmup):
    res = {k: [] for k in trees}
    for _ in range(runs):
        for name, tree in trees.items():
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"bench.py failed in {tree}:\n{p.stderr[-2000:]}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            rec = json.loads(line)
            res[name].append(float(rec.get("clips_per_s", rec.get("value"))))
    return {k: {"clips_per_s": v, "median": statistics.median(v), "spread": max(v) - min(v)} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50, help="calls between the two events of one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-tree", default=None, help="a built tree of the parent commit: bench.py runs there too")
    ap.add_argument("--bench-runs", type=int, default=3, help="bench.py runs per tree (0: skip)")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/data_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    B, T, H, W, S = 4, 8, 256, 341, 256
    out = {"tool": "data_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.steps,
           "warmup": args.warmup, "build": build_stamp.current()}
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, clips_per_video=(B,), sizes=((H, W),), test_clips=1, seed=0)
        cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.SYNTHETIC_DATA", False, "CSTS_AMD.DATA_ROOT", root,
                               "DATA.TRAIN_CROP_SIZE", S, "DATA.TEST_CROP_SIZE", S])
        store = D.ClipStore(cfg, "train", dev)
    store.upload()
    loader = D.ClipLoader(store, batch=B, seed=1)
    ids, tab = loader.table(np.arange(B))
    tab_dev = torch.from_numpy(tab).to(dev)
    key = torch.tensor([0x5EED], dtype=torch.int64, device=dev)
    kw = loader.spatial_args()
    idx = tab_dev[:, 7 + T:7 + 2 * T].to(torch.int32)
    cen = tab_dev[:, 7 + 2 * T:].to(torch.int32)
    labels = store.labels[tab_dev[:, 7:7 + T]]
    recs = [torch.from_numpy(store.frames_host[i]).to(dev) for i in ids]
    specs = [torch.from_numpy(store.spec_host[i][:, :store.usable[i]].copy()).to(dev) for i in ids]

    def composition():
        video, audio, lab, hm = [], [], [], []
        lbl = lib.load()
        for b in range(B):
            # clip b must draw u[b]: the rule of the whole batch runs per clip and row b is kept
            par = torch.empty(B, 5, dtype=torch.int32, device=dev)
            new = torch.empty_like(labels)
            lib.check(lbl.csts_spatial_params(key.data_ptr(), labels.data_ptr(), B, T, labels.shape[2], H, W, S, kw["min_scale"],
                                              kw["max_scale"], -1, int(kw["random_flip"]), int(kw["inverse_uniform"]), par.data_ptr(),
                                              new.data_ptr(), torch.cuda.current_stream().cuda_stream), "csts_spatial_params")
            video.append(inputs.clip_sample(recs[b], idx[b:b + 1], par[b:b + 1], S))
            audio.append(inputs.audio_windows_at(specs[b], cen[b:b + 1], 256))
            lab.append(new[b:b + 1])
            hm.append(inputs.gaze_heatmaps(new[b:b + 1], H=S // 4, W=S // 4))
        return {"video": torch.cat(video), "audio": torch.cat(audio), "labels": torch.cat(lab), "labels_hm": torch.cat(hm)}

    g_loader, a = graphed(lambda: loader.assemble(tab_dev, tab, key))
    g_comp, b = graphed(composition)
    g_loader.replay()
    g_comp.replay()
    torch.cuda.synchronize()
    same = {k: bool(torch.equal(a[k], b[k])) for k in ("video", "audio", "labels", "labels_hm")}
    variants = {"loader_graph": g_loader.replay, "composition_graph": g_comp.replay, "composition_eager": composition,
                "loader_eager": lambda: loader.assemble(tab_dev, tab, key)}
    res = alternate(variants, args.warmup, args.steps, args.rounds)
    written = B * (3 * T * S * S + T * S * S + T * (S // 4) ** 2) * 4
    out["batch"] = {"B": B, "T": T, "H": H, "W": W, "S": S, "bit_equal": same, **res,
                    "written_MB": round(written / 1e6, 2),
                    "loader_graph_GBps": round(written / res["loader_graph"]["median_us"] / 1e3, 1),
                    "composition_graph_over_loader_graph": round(res["composition_graph"]["median_us"] / res["loader_graph"]["median_us"], 3)}
    if args.bench_runs > 0:
        trees = {"this": ROOT}
        if args.parent_tree:
            trees["parent"] = os.path.abspath(args.parent_tree)
        out["bench"] = bench_runs(trees, args.bench_runs, args.bench_steps, args.bench_warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
