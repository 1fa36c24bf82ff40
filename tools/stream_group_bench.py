"""Many live streams on one device, measured ("Stream group").  Every step runs in a child process of its own under a
time limit of its own, and the steps stop at the first one that fails:

  replay N   N recordings of 1088 x 1080 replayed at one frame per tick with the matching audio (stride 9, bf16), through
             (group)  one GazePredictor.stream_group(N, batch=min(N, 4)), one push per tick, and
             (single) N independent GazePredictor.stream(batch=1) objects pushed in turn -- what the repository offered before;
             alternated over several rounds, every tick timed on the host with the device drained.  Reports windows/s and the
             per-tick time of both, and, counted on the host in a replay of its own, per tick: the kernel-library entries called
             (each is one launch; torch's own copies and concatenations are not counted), the host-to-device copies and the
             predict_batch calls.
  forward    the forward-only rate of predict_batch at b = 1, 2, 4 on synthetic batches (graph replay), alternated over rounds.
  neighbours whether a window's bits change when its batch neighbours change, at the same batch size (b = 2 and b = 4).
  bench      `python bench.py --gpus 1` on this tree, and on a build of the parent commit when --parent DIR names one, alternated;
             clips/s of every run and the run-to-run spread.

    python tools/stream_group_bench.py [--parent DIR]             # -> profiles/stream_group_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
PER, H, W, STRIDE, POOL = 800, 1088, 1080, 9, 8     # samples per frame; the source size; the frames a recording cycles through
TICKS = 86 + 9 * 10                                 # windows 0..10 of every stream


class Counts:
    """Counts, while active: the kernel-library entries called (lib.check sees every one), the tensors that went from the host to
    the device (torch.tensor(..., device=cuda) and Tensor.to of a host tensor) and the predict_batch calls."""

    def __init__(self, predictor):
        self.predictor, self.entries, self.h2d, self.forwards = predictor, 0, 0, 0

    def __enter__(self):
        import torch
        from csts_amd import lib
        self._check, self._tensor, self._to, self._predict = lib.check, torch.tensor, torch.Tensor.to, self.predictor.predict_batch

        def check(rc, name=None, *a, **k):
            self.entries += 1
            return self._check(rc, name, *a, **k)

        def tensor(*a, **k):
            out = self._tensor(*a, **k)
            self.h2d += int(out.is_cuda)
            return out

        def to(t, *a, **k):
            out = self._to(t, *a, **k)
            self.h2d += int(out.is_cuda and not t.is_cuda)
            return out

        def predict(*a, **k):
            self.forwards += 1
            return self._predict(*a, **k)

        lib.check, torch.tensor, torch.Tensor.to, self.predictor.predict_batch = check, tensor, to, predict
        return self

    def __exit__(self, *exc):
        import torch
        from csts_amd import lib
        lib.check, torch.tensor, torch.Tensor.to = self._check, self._tensor, self._to
        del self.predictor.predict_batch

    def per_tick(self, ticks):
        return {"library_entries": round(self.entries / ticks, 2), "host_to_device_copies": round(self.h2d / ticks, 2),
                "forwards": round(self.forwards / ticks, 3)}


def _predictor(compute):
    import torch
    from csts_amd import GazePredictor
    from csts_amd.config import load_yaml
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", compute])
    torch.manual_seed(cfg.RNG_SEED)
    return cfg, GazePredictor(cfg, device=torch.device("cuda:0"), graph=True)


def step_replay(args):
    import torch
    dev = torch.device("cuda:0")
    _, predictor = _predictor(args.compute)
    n, batch = args.n, min(args.n, 4)
    g = torch.Generator(device=dev).manual_seed(args.n)
    frames = [torch.randint(0, 256, (POOL, H, W, 3), generator=g, device=dev, dtype=torch.uint8) for _ in range(n)]
    wavs = [0.1 * torch.randn(TICKS * PER, generator=g, device=dev) for _ in range(n)]

    def piece(i, t):
        return frames[i][t % POOL:t % POOL + 1], wavs[i][t * PER:(t + 1) * PER]

    def run_group():
        group = predictor.stream_group(n, stride=STRIDE, batch=batch)
        secs, windows = [], 0
        for t in range(TICKS):
            t0 = time.perf_counter()
            res = group.push({i: piece(i, t) for i in range(n)})
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            windows += sum(len(rs) for rs in res.values())
        return secs, windows

    def run_single():
        streams = [predictor.stream(stride=STRIDE, batch=1) for _ in range(n)]
        secs, windows = [], 0
        for t in range(TICKS):
            t0 = time.perf_counter()
            for i, s in enumerate(streams):
                windows += len(s.push(*piece(i, t)))
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return secs, windows

    variants = {"group": run_group, "single": run_single}
    counts = {}
    for name, run in variants.items():                          # warm-up (captures the graphs), then the counts in a replay of
        run()                                                   # their own: a capture calls every entry of a forward once
        with Counts(predictor) as c:
            _, windows = run()
        assert windows == n * 11, (name, windows)
        counts[name] = c.per_tick(TICKS)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, run in variants.items():
            times[name].append(run()[0])

    def summary(rounds):
        total = [sum(r) for r in rounds]
        busy = [statistics.mean(sorted(r)[-11:]) for r in rounds]               # the 11 ticks in which windows run
        return {"windows_per_s": round(n * 11 / statistics.median(total), 2),
                "windows_per_s_rounds": [round(n * 11 / v, 2) for v in total],
                "tick_mean_ms": round(statistics.median([statistics.mean(r) for r in rounds]) * 1e3, 3),
                "tick_median_ms": round(statistics.median([statistics.median(r) for r in rounds]) * 1e3, 3),
                "tick_with_windows_mean_ms": round(statistics.median(busy) * 1e3, 3)}

    res = {name: dict(summary(times[name]), per_tick=counts[name]) for name in variants}
    return {"streams": n, "batch": batch, "ticks": TICKS, "windows": n * 11, "rounds": args.rounds, **res,
            "group_over_single_windows_per_s": round(res["group"]["windows_per_s"] / res["single"]["windows_per_s"], 3)}


def step_forward(args):
    import torch
    from csts_amd import train as T
    dev = torch.device("cuda:0")
    cfg, predictor = _predictor(args.compute)
    batches = {b: T.synthetic_batch(b, cfg.DATA.NUM_FRAMES, cfg.DATA.TEST_CROP_SIZE, 2000 + b, dev, spatial=T.spatial_config(cfg, train=False))
               for b in (1, 2, 4)}
    iters = 100
    for b, x in batches.items():
        for _ in range(10):
            predictor.predict_batch(x)
    torch.cuda.synchronize()
    rates = {b: [] for b in batches}
    for _ in range(args.rounds):
        for b, x in batches.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                predictor.predict_batch(x)
            torch.cuda.synchronize()
            rates[b].append(b * iters / (time.perf_counter() - t0))
    out = {f"b{b}": {"clips_per_s": round(statistics.median(v), 1), "rounds": [round(r, 1) for r in v],
                     "ms_per_forward": round(1e3 * b / statistics.median(v), 3)} for b, v in rates.items()}
    out["b4_over_b1"] = round(out["b4"]["clips_per_s"] / out["b1"]["clips_per_s"], 3)
    out["b2_over_b1"] = round(out["b2"]["clips_per_s"] / out["b1"]["clips_per_s"], 3)
    out["iterations"] = iters
    return out


def step_neighbours(args):
    import torch
    from csts_amd import train as T
    dev = torch.device("cuda:0")
    cfg, predictor = _predictor(args.compute)
    pool = T.synthetic_batch(8, cfg.DATA.NUM_FRAMES, cfg.DATA.TEST_CROP_SIZE, 2100, dev, spatial=T.spatial_config(cfg, train=False))
    out = {}
    for b in (2, 4):
        changed = False
        for row in range(b):                                     # the same clip in row `row`, other clips around it
            a_idx = list(range(b))
            b_idx = [i if i == row else i + 4 for i in range(b)]
            ra = predictor.predict_batch({k: pool[k][a_idx] for k in ("video", "audio")})
            rb = predictor.predict_batch({k: pool[k][b_idx] for k in ("video", "audio")})
            assert not torch.equal(ra["heatmaps"], rb["heatmaps"])
            changed |= any(not torch.equal(ra[k][row], rb[k][row]) for k in ("points", "peak", "heatmaps", "rescaled"))
        out[f"b{b}_bits_change_with_neighbours"] = bool(changed)
    return out


def step_bench(args):
    trees = {"this": ROOT}
    if args.parent:
        trees["parent"] = os.path.abspath(args.parent)
    runs = {name: [] for name in trees}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
    for _ in range(args.rounds):
        for name, tree in trees.items():
            p = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=tree, capture_output=True, text=True)
            if p.returncode != 0:
                raise SystemExit(f"bench.py in {name} ended with {p.returncode}: {p.stderr[-2000:]}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            runs[name].append(json.loads(line)["value"])
    out = {"command": " ".join(cmd[1:]), "unit": "clips/s"}
    for name, v in runs.items():
        out[name] = {"runs": v, "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}
    if "parent" in runs:
        out["this_over_parent_median"] = round(out["this"]["median"] / out["parent"]["median"], 4)
    else:
        out["parent"] = "not measured"
    return out


STEPS = {"replay": step_replay, "forward": step_forward, "neighbours": step_neighbours, "bench": step_bench}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS), help="run one step in this process and print its JSON (the driver's children)")
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"])
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit, for the bench step")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--skip", nargs="*", default=[], choices=sorted(STEPS))
    ap.add_argument("--limit", type=int, default=420, help="seconds every step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_group_bench.json"))
    args = ap.parse_args()
    if args.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/stream_group_bench.py measures on an MI355X: no GPU found")
        print("step_json: " + json.dumps(STEPS[args.step](args)), flush=True)
        return
    import build_stamp
    out = {"tool": "stream_group_bench", "compute": args.compute, "source": [H, W], "stride": STRIDE, "build": build_stamp.current()}
    common = ["--rounds", str(args.rounds), "--compute", args.compute, "--bench-steps", str(args.bench_steps), "--bench-warmup",
              str(args.bench_warmup)] + (["--parent", args.parent] if args.parent else [])
    plan = [("replay", ["--n", str(n)], f"replay_{n}") for n in args.streams] + [(s, [], s) for s in ("forward", "neighbours", "bench")]
    for step, extra, key in plan:
        if step in args.skip:
            continue
        limit = args.limit * (2 * args.rounds + 1 if step == "bench" else 1)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + extra + common,
                           cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("step_json: ")]
        if p.returncode != 0 or not lines:                       # nothing more is started on the device after a step that failed
            out[key] = {"failed": p.returncode, "stderr": p.stderr[-2000:]}
            out["stopped_after"] = key
            break
        out[key] = json.loads(lines[-1][len("step_json: "):])
        print(f"{key}: {lines[-1][len('step_json: '):]}", flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))
    if "stopped_after" in out:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
