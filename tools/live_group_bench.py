"""The live track of many streams on one device, measured ("Live group").  Every step runs in a child process of its
own under a time limit of its own, and the steps stop at the first one that fails:

  replay N   N recordings of 1088 x 1080 replayed at one frame per tick with the matching audio (stride 9, bf16, live="linear"),
             every frame answered when it arrives, through
             (group)  one GazePredictor.live_group(N, batch=min(N, 4)), one push_live per tick, and
             (single) N independent GazePredictor.stream(live=..., batch=1) objects pushed in turn -- what the repository offered
                      before;
             each with and without overlay=True, alternated over several rounds, every tick timed on the host with the device
             drained.  Reports frames answered per second, windows per second and the per-tick time of each, and, counted on the
             host in a replay of its own, per tick: the calls of ops.group_live_add and ops.group_live_rows (one launch each), of
             ops.live_track_add and ops.live_track_rows, and all kernel-library entries.
  bench      `python bench.py --gpus 1` on this tree, and on a build of the parent commit when --parent DIR names one, alternated;
             clips/s of every run and the run-to-run spread.

    python tools/live_group_bench.py [--parent DIR]               # -> profiles/live_group_bench.json
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

from stream_group_bench import H, PER, POOL, STRIDE, TICKS, W, YAML, _predictor, step_bench  # noqa: E402,F401

LIVE = "linear"
TRACK_OPS = ("group_live_add", "group_live_rows", "live_track_add", "live_track_rows")


class Counts:
    """Counts, while active: the calls of the four live-track functions of csts_amd.ops (each is one launch) and all the
    kernel-library entries called (lib.check sees every one)."""

    def __init__(self):
        self.calls, self.entries = dict.fromkeys(TRACK_OPS, 0), 0

    def __enter__(self):
        from csts_amd import lib, ops
        self._saved = {name: getattr(ops, name) for name in TRACK_OPS}
        self._check = lib.check

        def counted(name):
            def call(*a, **k):
                self.calls[name] += 1
                return self._saved[name](*a, **k)
            return call

        def check(rc, name=None, *a, **k):
            self.entries += 1
            return self._check(rc, name, *a, **k)

        for name in TRACK_OPS:
            setattr(ops, name, counted(name))
        lib.check = check
        return self

    def __exit__(self, *exc):
        from csts_amd import lib, ops
        for name, fn in self._saved.items():
            setattr(ops, name, fn)
        lib.check = self._check

    def per_tick(self, ticks):
        out = {name: round(v / ticks, 3) for name, v in self.calls.items()}
        out["library_entries"] = round(self.entries / ticks, 2)
        return out


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

    def run_group(overlay):
        group = predictor.live_group(n, LIVE, stride=STRIDE, batch=batch, overlay=overlay)
        secs, windows, answered = [], 0, 0
        for t in range(TICKS):
            t0 = time.perf_counter()
            res, live = group.push_live({i: piece(i, t) for i in range(n)})
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            windows += sum(len(rs) for rs in res.values())
            answered += sum(rows["frame_idx"].numel() for rows in live.values())
        return secs, windows, answered

    def run_single(overlay):
        streams = [predictor.stream(stride=STRIDE, batch=1, live=LIVE, overlay=overlay) for _ in range(n)]
        secs, windows, answered = [], 0, 0
        for t in range(TICKS):
            t0 = time.perf_counter()
            for i, s in enumerate(streams):
                res, rows = s.push_live(*piece(i, t))
                windows += len(res)
                answered += rows["frame_idx"].numel()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return secs, windows, answered

    variants = {"group": lambda: run_group(False), "single": lambda: run_single(False),
                "group_overlay": lambda: run_group(True), "single_overlay": lambda: run_single(True)}
    counts = {}
    for name, run in variants.items():                          # warm-up (captures the graphs), then the counts in a replay of
        run()                                                   # their own
        with Counts() as c:
            _, windows, answered = run()
        assert windows == n * 11 and answered == n * TICKS, (name, windows, answered)
        counts[name] = c.per_tick(TICKS)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, run in variants.items():
            times[name].append(run()[0])

    def summary(rounds):
        total = [sum(r) for r in rounds]
        return {"frames_per_s": round(n * TICKS / statistics.median(total), 1),
                "frames_per_s_rounds": [round(n * TICKS / v, 1) for v in total],
                "windows_per_s": round(n * 11 / statistics.median(total), 2),
                "tick_mean_ms": round(statistics.median([statistics.mean(r) for r in rounds]) * 1e3, 3),
                "tick_median_ms": round(statistics.median([statistics.median(r) for r in rounds]) * 1e3, 3)}

    res = {name: dict(summary(times[name]), per_tick=counts[name]) for name in variants}
    return {"streams": n, "batch": batch, "live": LIVE, "ticks": TICKS, "frames": n * TICKS, "windows": n * 11, "rounds": args.rounds,
            **res,
            "group_over_single_frames_per_s": round(res["group"]["frames_per_s"] / res["single"]["frames_per_s"], 3),
            "group_over_single_frames_per_s_overlay": round(res["group_overlay"]["frames_per_s"] / res["single_overlay"]["frames_per_s"], 3)}


STEPS = {"replay": step_replay, "bench": step_bench}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_group_bench.json"))
    args = ap.parse_args()
    if args.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/live_group_bench.py measures on an MI355X: no GPU found")
        print("step_json: " + json.dumps(STEPS[args.step](args)), flush=True)
        return
    import build_stamp
    out = {"tool": "live_group_bench", "compute": args.compute, "source": [H, W], "stride": STRIDE, "live": LIVE,
           "build": build_stamp.current()}
    common = ["--rounds", str(args.rounds), "--compute", args.compute, "--bench-steps", str(args.bench_steps), "--bench-warmup",
              str(args.bench_warmup)] + (["--parent", args.parent] if args.parent else [])
    plan = [("replay", ["--n", str(n)], f"replay_{n}") for n in args.streams] + [("bench", [], "bench")]
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
