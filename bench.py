#!/usr/bin/env python3
"""bench.py -- CSTS throughput on MI355X (BASELINE.json metric: clips/s, training step; --mode fwd: forward only).

    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: starts its own N ranks, self_launch)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (config.workload): CSTS_Ego4D_Gaze_Forecast.yaml + MODEL.LOSS_FUNC kldiv+egonce, 16 frames x 256^2
(the reference itself cannot run 224^2; --crop 224 runs the labelled, parity-unpinned extension),
b = 4 clips per GPU (weak scaling), bf16 MFMA mode with fp32 residual stream, synthetic clips + 24 kHz STFT resident
in HBM before the timed region.

--mode train (default, BASELINE config 3/4): one step = forward + KLDiv + 0.05 EgoNCE + backward (+ RCCL gradient
all-reduce when N > 1) + L2 clip + AdamW: nothing of the reference iteration (train_avgaze_net.py:65-109) is skipped.
N = 1 replays the whole iteration as ONE HIP graph; N > 1 replays a chain of graphs with the collectives issued
eagerly between them (csts_amd.train.SegmentedTrainStep).
--mode fwd (BASELINE config 2): eval-mode forward + frame_softmax of the same batch, one HIP graph.

Timing: W untimed steps, then EXACTLY K steps between barrier + synchronize, max over ranks -> `value`.  A plain run does
nothing else: set up, warm up, time the K steps, write --dump-outputs, and rank 0 prints ONE JSON line.

--dump-outputs DIR: right after the K timed steps, rank 0 writes what the last of them gave its caller as DIR/<name>.npy
(float32, float64 kept; at most 16 MB per array; train: loss, kld, nce and a seeded sample of the updated parameters; fwd: heat maps and embeddings; see
step_outputs).  Weights and batch are drawn from fixed seeds, so two builds run with the same arguments see the same inputs.

--full adds what the headline does not need (each one can be switched off with its --no-* option):
`loss_check` compares the eval-mode loss of THIS model on the seed-1000 batch with the value the imported reference gave
for the same weights and batch (tests/golden/bench_expected.json) and fails the run when they disagree; after the timed
steps, `median_step_ms` = median of >= 50 single steps timed with HIP events after >= 10 warm-up steps; `fwd_ms` /
`loss_ms` / `bwd_ms` / `optimizer_ms` (N = 1, train) = medians of the graph chain's segments; "roofline" for the dominant
kernel, measured live with HIP events on the launch stream over an instrumented pass (--op-breakdown, --dump-gemm and
--dump-gemm-order write from that pass); and "cpu_baseline" = the CPU oracle (a port, plain PyTorch fp32) timed on the
host cores on a bounded sample of the same workload (rank 0, N = 1 only).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))      # tools/work_model.py: algorithmic bytes / flop per C-ABI entry

import torch  # noqa: E402

FWD_GFLOP_PER_CLIP = {8: 208.7, 16: 465.3, 32: 1122.3}      # SURVEY.md 8(d) / BASELINE.md section 2 (256^2)
BYTES_FWD_GB_PER_CLIP = {8: 1.24, 16: 2.34, 32: 4.53}
PEAK_BF16_TFLOPS = 2500.0                                     # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--mode", default="train", choices=["train", "fwd"])
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--crop", type=int, default=256, choices=[256, 224],
                   help="224 = labelled EXTENSION (fusion kernels follow the final grid, parity unpinned: the reference rejects it)")
    p.add_argument("--batch-per-gpu", type=int, default=4)
    p.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"],
                   help="bf16: the headline mode; fp32: the parity-certified mode; fp16: the reference's autocast arithmetic + dynamic loss scaling")
    p.add_argument("--full", action="store_true",
                   help="also run the loss check, median_step_ms, the segment split, the roofline pass and the CPU baseline "
                        "(the --no-* options below switch single ones off)")
    p.add_argument("--median-steps", type=int, default=50, help="--full: single steps timed with HIP events for median_step_ms")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--quick-cpu-baseline", action="store_true", help="--full: only the headline CPU sample (B=2 at the benchmarked grid)")
    p.add_argument("--no-roofline", action="store_true")
    p.add_argument("--no-segments", action="store_true", help="skip the forward / backward / optimizer split (N = 1, train)")
    p.add_argument("--no-loss-check", action="store_true")
    p.add_argument("--rehearse-dist", action="store_true",
                   help="run the N>1 code path (RCCL process group, graph chain + eager collectives) with ONE rank")
    p.add_argument("--trunk-cut", type=int, default=None,
                   help="data-parallel graph chain: second autograd cut in front of this video block (default CSTS_AMD.TRUNK_CUT = 3; 0 = off)")
    p.add_argument("--bucket-dtype", default=None, choices=["fp32", "bf16", "fp16"],
                   help="data-parallel gradient buckets: fp32 (default) or the 16-bit type of the compute mode (half the xGMI bytes)")
    p.add_argument("--no-grad-factors", action="store_true",
                   help="data-parallel chain: all-reduce the fusion-conv weight gradients (151 MB each) instead of all-gathering their rank-(B T') factors")
    p.add_argument("--eager-dist", action="store_true",
                   help="N>1: the eager step with hook-driven gradient buckets (GradAllReduce) instead of the graph chain")
    p.add_argument("--no-graph", action="store_true", help="do not capture anything into HIP graphs")
    p.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                   help="gloo: control-flow rehearsal of the N>1 path with several ranks on ONE GPU (RCCL refuses two ranks per device)")
    p.add_argument("--op-breakdown", default=None, help="write per-C-ABI-entry device time of one eager step to this file")
    p.add_argument("--dump-gemm", default=None, help="write a per-shape GEMM timing table to this file")
    p.add_argument("--dump-gemm-order", default=None,
                   help="write the ORDERED list of one step's GEMM launches (kernel name, shape, event-timed us) as JSON: "
                        "tools/trace_gemm_map.py zips it with a rocprofv3 kernel trace of the graph replay")
    p.add_argument("--one-stream", action="store_true", help="audio trunk on the video trunk's stream (CSTS_AMD.TWO_STREAMS False)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed step gave its caller as DIR/<name>.npy (rank 0; see step_outputs)")
    args = p.parse_args()
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full and (args.op_breakdown or args.dump_gemm or args.dump_gemm_order):
        p.error("--op-breakdown, --dump-gemm and --dump-gemm-order come from the roofline pass: add --full")
    return args


class GemmTimer:
    """HIP-event timing of every csts_gemm call at the C-ABI boundary (events recorded on the launch stream = torch's
    current stream).  Each call is attributed to the kernel csts_gemm picks for it (csts_gemm_plan), named exactly as
    rocprofv3 prints it, so the live numbers can be checked against profiles/*_kernel_stats.csv."""

    class _Proxy:
        def __init__(self, lib, owner):
            self._lib, self._owner = lib, owner

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if name != "csts_gemm":
                return fn
            owner, lib = self._owner, self._lib

            def timed(argsref, stream):
                import ctypes as C
                a = argsref._obj
                name_buf = C.create_string_buffer(160)
                ns = C.c_int()
                lib.csts_gemm_kernel_name(argsref, name_buf, 160, C.byref(ns))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(argsref, stream)
                e1.record()
                esz = lambda dt: 4 if dt == 0 else 2
                byt = a.M * a.K * esz(a.a_dt) + a.N * a.K * esz(a.b_dt) + a.M * a.N * esz(a.c_dt)     # A + B + C once
                ext = 0                                            # compulsory epilogue operands on top of A + B + C
                if a.aux:
                    ext += a.M * a.N * esz(a.aux_dt)               # GELU pre-activation written / read
                if a.residual:
                    ext += (a.res_row_mod if a.res_row_mod else a.M) * a.N * esz(a.r_dt)
                owner.records.append((name_buf.value.decode(), ns.value, 2.0 * a.M * a.N * a.K, byt, e0, e1,
                                      (a.layout, a.M, a.N, a.K, ns.value), ext))
                owner.args.append(type(a).from_buffer_copy(a))
                return rc
            return timed

    def __init__(self):
        self.records = []   # (kernel name, nsplit, flops, bytes, ev0, ev1, shape)
        self.args = []      # a copy of every call's csts_gemm_args (replay_kernel re-issues them on scratch operands)

    def replay_kernel(self, name, steps, replays=7, nsets=3):
        """Average launch duration of kernel `name` INSIDE A HIP-GRAPH REPLAY: the launches it had in the last instrumented step
        (same shapes, leading dimensions, dtypes and epilogues, in step order) are re-issued on scratch operands -- rotating
        over `nsets` operand sets per shape, so that a launch does not find its operands in L2 from the launch before it --
        captured into ONE graph and replayed; HIP events bracket each replay on the launch stream.  Returns
        (launches, seconds per replay [median], seconds per replay [min])."""
        import ctypes as C
        from csts_amd import lib as L
        lib = L.load()
        n = len(self.records) // steps
        sel = [a for (nm, *_), a in zip(self.records[-n:], self.args[-n:]) if nm == name and a.layout == 0 and a.split_k <= 1]
        if not sel:
            return 0, None, None
        dev = torch.device("cuda", torch.cuda.current_device())
        from csts_amd import lib as _L
        tdt = lambda dt: torch.float32 if dt == 0 else _L.half_dtype()
        pool, rot = {}, {}

        def buf(key, numel, dt, fill):
            k = (key, numel, dt)
            if k not in pool:
                t = torch.empty(numel, dtype=tdt(dt), device=dev)
                t.normal_(0.0, fill) if fill else t.zero_()
                pool[k] = t
            return pool[k].data_ptr()

        calls = []
        for a in sel:
            sig = (a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.a_dt, a.b_dt, a.c_dt, a.epilogue, bool(a.aux), bool(a.residual), a.res_row_mod)
            r = rot[sig] = (rot.get(sig, -1) + 1) % nsets
            b = type(a).from_buffer_copy(a)
            b.A = buf(("A", sig, r), a.M * a.lda, a.a_dt, 1.0)
            b.B = buf(("B", sig, r), a.N * a.ldb, a.b_dt, 0.05)
            b.C = buf(("C", sig, r), a.M * a.ldc, a.c_dt, 0.0)
            b.bias = buf(("bias", sig, 0), a.N, 0, 0.1) if a.bias else None
            b.aux = buf(("aux", sig, r), a.M * a.ldaux, a.aux_dt, 1.0) if a.aux else None
            b.residual = buf(("res", sig, r), (a.res_row_mod or a.M) * a.ldr, a.r_dt, 1.0) if a.residual else None
            if a.row_scale:
                rows = (a.M + a.rows_per_scale - 1) // max(a.rows_per_scale, 1)
                k = (("rs", sig), rows, 0)
                if k not in pool:
                    pool[k] = torch.ones(rows, dtype=torch.float32, device=dev)
                b.row_scale = pool[k].data_ptr()
            b.workspace, b.ws_bytes, b.colsum = None, 0, None
            calls.append(b)
        def issue():
            st = torch.cuda.current_stream().cuda_stream          # inside torch.cuda.graph(...) this is the capturing stream
            for b in calls:
                if lib.csts_gemm(C.byref(b), st) != 0:
                    raise RuntimeError("csts_gemm failed in the graph-replay roofline pass: " + lib.csts_last_error().decode())
        issue()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            issue()
        times = []
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        del g
        pool.clear()
        return len(calls), statistics.median(times[1:]), min(times[1:])

    def install(self):
        from csts_amd import lib as L
        self._orig = L.load()
        L._lib = GemmTimer._Proxy(self._orig, self)

    def remove(self):
        from csts_amd import lib as L
        L._lib = self._orig

    def summary(self):
        """kernel name -> [launches, flops, bytes, seconds, has_finish_pass]"""
        torch.cuda.synchronize()
        agg = {}
        for name, ns, fl, by, e0, e1, _shape, ext in self.records:
            a = agg.setdefault(name, [0, 0.0, 0.0, 0.0, False, 0.0])
            a[0] += 1
            a[1] += fl
            a[2] += by
            a[3] += e0.elapsed_time(e1) * 1e-3
            a[4] = a[4] or ns > 1
            a[5] += ext
        return agg

    def dump_order(self, path, steps):
        """The launches of the LAST instrumented step, in issue order."""
        torch.cuda.synchronize()
        n = len(self.records) // steps
        rows = [{"kernel": name, "split": ns, "layout": "NT NN TN".split()[shape[0]], "M": shape[1], "N": shape[2], "K": shape[3],
                 "flop": fl, "bytes": by, "epilogue_bytes": ext, "us_eager_events": round(e0.elapsed_time(e1) * 1e3, 2)}
                for name, ns, fl, by, e0, e1, shape, ext in self.records[-n:]]
        with open(path, "w") as f:
            json.dump(rows, f)

    def dump_shapes(self, path):
        torch.cuda.synchronize()
        per = {}
        for name, ns, fl, by, e0, e1, shape, ext in self.records:
            a = per.setdefault(shape + (name,), [0, 0.0, fl, by])
            a[0] += 1
            a[1] += e0.elapsed_time(e1) * 1e-3
        rows = sorted(per.items(), key=lambda kv: -kv[1][1])
        with open(path, "w") as f:
            f.write("layout M N K split calls total_ms avg_us TFLOPs GBps kernel\n")
            for (lay, M, N, K, sp, name), (n, sec, fl, by) in rows:
                f.write(f"{'NT NN TN'.split()[lay]} {M} {N} {K} {sp} {n} {sec*1e3:.3f} {sec/n*1e6:.1f} {fl*n/sec/1e12:.1f} {by*n/sec/1e9:.0f} {name}\n")


def _work(name, args):
    if name == "csts_gemm":
        a = args[0]._obj
        esz = lambda dt: 4 if dt == 0 else 2
        byt = a.M * a.K * esz(a.a_dt) + a.N * a.K * esz(a.b_dt) + a.M * a.N * esz(a.c_dt)
        if a.aux:
            byt += a.M * a.N * esz(a.aux_dt)
        if a.residual:
            byt += (a.res_row_mod if a.res_row_mod else a.M) * a.N * esz(a.r_dt)
        return byt, 2.0 * a.M * a.N * a.K
    import work_model
    return work_model.work(name, args)


class OpTimer:
    """HIP-event timing of EVERY C-ABI entry point (per-family device time of one eager single-stream step)."""

    class _Proxy:
        def __init__(self, lib, rec):
            self._lib, self._rec = lib, rec

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith("csts_") or name.endswith("_workspace") or name in (
                    "csts_last_error", "csts_abi_version", "csts_gemm_v2_eligible", "csts_gemm_kernel_name", "csts_gemm_plan",
                    "csts_stft_frames"):
                return fn
            rec = self._rec

            def timed(*a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*a)
                e1.record()
                rec.append((name, e0, e1, _work(name, a)))
                return rc
            return timed

    def __init__(self):
        self.rec = []

    def install(self):
        from csts_amd import lib as L
        self._orig = L.load()
        L._lib = OpTimer._Proxy(self._orig, self.rec)

    def remove(self):
        from csts_amd import lib as L
        L._lib = self._orig

    def summary(self, steps, extra_work=None):
        """Per C-ABI entry: calls, device ms (HIP events around each call of an eager single-stream step: 8-12 % above the
        graph replay), and -- where tools/work_model.py knows the entry -- the ALGORITHMIC bytes / flop of those calls (every
        operand once) with the roofline fractions they give: bytes / ms / 8 TB/s, flop / ms / 2.5 PF.
        extra_work: {entry: (bytes, flop)} for entries whose work is not visible in the call arguments (grouped weight
        gradients: device item tables; the optimizer: device tensor tables)."""
        torch.cuda.synchronize()
        agg = {}
        for name, e0, e1, w in self.rec:
            a = agg.setdefault(name[5:], [0, 0.0, 0.0, 0.0, True])
            a[0] += 1
            a[1] += e0.elapsed_time(e1)
            if w is None:
                a[4] = False
            else:
                a[2] += w[0]
                a[3] += w[1]
        for k, (b, f) in (extra_work or {}).items():
            if k in agg:
                agg[k][2], agg[k][3], agg[k][4] = b * steps, f * steps, True
        out = {}
        for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            d = {"calls": v[0] // steps, "ms": round(v[1] / steps, 3)}
            if v[4] and v[1] > 0 and (v[2] > 0 or v[3] > 0):
                sec = v[1] / 1e3
                d["algorithmic_bytes"] = int(v[2] / steps)
                d["algorithmic_flop"] = int(v[3] / steps)
                d["hbm_frac"] = round(v[2] / sec / 8e12, 4)
                d["mfma_frac"] = round(v[3] / sec / 2.5e15, 4)
                d["bound"] = "hbm" if d["hbm_frac"] >= d["mfma_frac"] else "mfma"
            out[k] = d
        return out


# ------------------------------------------------------------------------------------------------ output dump
DUMP_MAX_ELEMS = 4 << 20        # one dumped array: at most 16 MB (a fixed, seeded sample of anything larger)
PARAM_SAMPLE = 16384            # elements per parameter tensor in params_sample.npy (the whole tensor when smaller)


def _sample(flat, n, g):
    """`n` elements of the 1-D tensor `flat` at indices drawn from the CPU generator `g` (sorted; same draw on every run)."""
    idx = torch.randint(0, flat.numel(), (n,), generator=g).sort().values
    return flat[idx.to(flat.device)]


def step_outputs(mode, res, core):
    """What a caller of the timed step received from its last run, copied to the host as (name, tensor) pairs.
    train: loss, kld, nce (the step's return value) and params_sample = the parameters that step updated, PARAM_SAMPLE
    seeded elements of every tensor concatenated in named_parameters() order (all 524 tensors are 753 MB).
    fwd: heatmaps (frame_softmax of the logits), video_embed, audio_embed."""
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        if mode == "fwd":
            out = list(zip(("heatmaps", "video_embed", "audio_embed"), res))
        else:
            out = [(n, t) for n, t in zip(("loss", "kld", "nce"), res) if t is not None]
            parts = []
            for _, p in core.named_parameters():
                flat = p.detach().reshape(-1)
                parts.append(_sample(flat, PARAM_SAMPLE, g) if flat.numel() > PARAM_SAMPLE else flat)
            out.append(("params_sample", torch.cat([t.float() for t in parts])))
        host = []
        for name, t in out:
            flat = t.detach().reshape(-1)
            if flat.numel() > DUMP_MAX_ELEMS:
                t = _sample(flat, DUMP_MAX_ELEMS, g)
            host.append((name, t.detach().to("cpu", torch.float64 if t.dtype == torch.float64 else torch.float32)))
    return host


def dump_outputs(path, arrays):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, t in arrays:
        np.save(os.path.join(path, name + ".npy"), t.numpy())


# ------------------------------------------------------------------------------------------------ CPU baseline
def _host_cpu():
    """(model string, physical cores visible to this process, logical CPUs visible to this process)."""
    model, phys = "unknown", set()
    try:
        allowed = os.sched_getaffinity(0)
    except AttributeError:
        allowed = set(range(os.cpu_count() or 1))
    try:
        cur = {}
        for line in open("/proc/cpuinfo"):
            if ":" not in line:
                if cur and int(cur.get("processor", -1)) in allowed:
                    phys.add((cur.get("physical id", "0"), cur.get("core id", cur.get("processor"))))
                cur = {}
                continue
            k, v = [t.strip() for t in line.split(":", 1)]
            cur[k] = v
            if k == "model name":
                model = v
        if cur and int(cur.get("processor", -1)) in allowed:
            phys.add((cur.get("physical id", "0"), cur.get("core id", cur.get("processor"))))
    except OSError:
        pass
    return model, max(1, len(phys) or len(allowed)), len(allowed)


def cpu_baseline(frames, mode, quick, budget_s=110.0, batch=4):
    """The CPU oracle (a port of the reference path to plain PyTorch fp32 ops, pinned to the reference by
    tests/test_oracle_golden.py) on the host cores: 1 warm-up + min of 3 per configuration.
    `value` = the train step (fwd + loss + bwd, no optimizer) -- or the forward in --mode fwd -- on THE GPU LINE'S OWN
    CONFIGURATION: the benchmarked token grid at the benchmarked per-GPU batch (16 x 256^2, B = 4 by default; 1 warm-up + min of
    2, ~40 s); the table adds 16 x 256^2 B = 2 and 8 x 256^2 at B = 1 / 2 / 4, forward and train, while the time budget lasts."""
    from oracle import csts_oracle as O
    model, phys, logical = _host_cpu()
    # these op sizes stop scaling well before a big host's core count (EPYC 9575F box: 26.8 s per 16x256^2 B=2 train step
    # with 128 threads, 10.6 s with 32): 32 threads, or every physical core when there are fewer
    threads = max(1, min(phys, logical, 32))
    torch.set_num_threads(threads)
    t_start = time.time()

    def run(T_, B, train, reps=3):
        P = O.seeded_params(T_, 256)
        if train:
            P = {k: v.requires_grad_(True) for k, v in P.items()}
        batch = O.synthetic_batch(B, T_, 256, seed=1000)
        best = None
        for it in range(reps + 1):
            t0 = time.time()
            if train:
                for v in P.values():
                    v.grad = None
                logits, ve, ae = O.csts_forward(P, batch["video"], batch["audio"], T_, 256, return_embed=True)
                loss, _, _ = O.csts_loss(logits, ve, ae, batch["labels_hm"], 0.05)
                loss.backward()
            else:
                with torch.no_grad():
                    O.csts_forward(P, batch["video"], batch["audio"], T_, 256, return_embed=True)
            dt = time.time() - t0
            if it > 0:                          # iteration 0 = warm-up
                best = dt if best is None else min(best, dt)
            if time.time() - t_start > budget_s and best is not None:
                break
        return best

    train = mode == "train"
    head = run(frames, batch, train, reps=2)
    out = {"value": round(batch / head, 4), "unit": "clips/s", "cores": threads, "kind": "port",
           "cpu_model": model, "physical_cores_visible": phys, "logical_cpus_visible": logical,
           "sample": f"CPU oracle (plain PyTorch fp32 ops), {'train step: fwd + KLDiv + 0.05 EgoNCE + bwd, no optimizer' if train else 'eval forward'}, "
                     f"B={batch}, {frames}x256^2 (the GPU line's configuration), 1 warm-up + min of 2: {head:.2f} s per step, {threads} threads"}
    if not quick:
        table = {f"{frames}x256^2 B={batch} {'train' if train else 'fwd'}": {"s_per_step": round(head, 3), "clips_per_s": round(batch / head, 3)}}
        if batch != 2 and time.time() - t_start < budget_s:
            t = run(frames, 2, train, reps=1)
            table[f"{frames}x256^2 B=2 {'train' if train else 'fwd'}"] = {"s_per_step": round(t, 3), "clips_per_s": round(2 / t, 3)}
        for B in (4, 2, 1):
            for what, tr in (("fwd", False), ("train", True)):
                if time.time() - t_start > budget_s:
                    break
                t = run(8, B, tr)
                table[f"8x256^2 B={B} {what}"] = {"s_per_step": round(t, 3), "clips_per_s": round(B / t, 3)}
        out["table"] = table
    out["wall_s"] = round(time.time() - t_start, 1)
    return out


# ------------------------------------------------------------------------------------------------ loss check
def loss_check(cfg, model, frames, b, crop, dev, T):
    """Eval-mode loss of this model (as built under torch.manual_seed(cfg.RNG_SEED)) on the CPU-generated seed-1000
    batch against the value the IMPORTED REFERENCE gave for the same weights and batch (oracle/gen_golden.py bench ->
    tests/golden/bench_expected.json).  A fingerprint of weights and batch guards the comparison: if this box draws other
    random numbers than the build container did, the check reports "unverifiable" instead of a false alarm."""
    path = os.path.join(ROOT, "tests", "golden", "bench_expected.json")
    key = f"T{frames}_B{b}"
    if crop != 256 or not os.path.exists(path):
        return {"status": "no reference value for this configuration"}
    exp = json.load(open(path)).get(key)
    if exp is None:
        return {"status": "no reference value for this configuration"}
    batch = T.synthetic_batch(b, frames, crop, exp["seed"], "cpu", pipeline="torch")
    sd = model.state_dict()
    fp = {n: float(sd[n].double().abs().sum()) for n in exp["fingerprint"] if not n.startswith("batch.")}
    for k in ("video", "audio", "labels_hm"):
        fp["batch." + k] = float(batch[k].double().abs().sum())
    same = all(abs(fp[n] - v) <= 1e-5 * max(abs(v), 1e-12) for n, v in exp["fingerprint"].items())
    was_training = model.training
    model.eval()
    from csts_amd import distributed as du
    with torch.no_grad(), du.local_only():      # only rank 0 comes here: no embedding all-gather
        bd = {k: v.to(dev) for k, v in batch.items()}
        loss, kld, nce, _ = T.compute_loss(cfg, model, bd["video"], bd["audio"], bd["labels_hm"])
        loss, kld, nce = float(loss), float(kld), float(nce)
    model.train(was_training)
    rel = abs(loss - exp["loss"]) / abs(exp["loss"])
    out = {"loss": round(loss, 6), "kld": round(kld, 6), "nce": round(nce, 5), "expected_loss": round(exp["loss"], 6),
           "expected_kld": round(exp["kld"], 6), "expected_nce": round(exp["nce"], 5), "rel_err": float(f"{rel:.3e}"),
           "tolerance": 1e-2 if cfg.CSTS_AMD.COMPUTE == "bf16" else 1e-4,
           "what": "eval-mode KLDiv + 0.05 EgoNCE of this model on the CPU-generated seed-1000 batch vs the imported reference "
                   "(same weights, same batch)"}
    if not same:
        out["status"] = "unverifiable: weights / batch drawn on this box differ from the build container's"
    else:
        out["status"] = "ok" if rel <= out["tolerance"] else "MISMATCH"
    return out


def self_launch(args):
    """`python bench.py --gpus N` with no launcher around it (no WORLD_SIZE in the environment): THIS process becomes the
    launcher.  It has not touched the GPU (torch.cuda.device_count() does not initialise HIP on this image) and never will:
    it starts N fresh children -- one rank per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment, the same
    command line -- waits for them and exits with the worst of their codes.  No exec from a process that holds the GPU.
    Fewer than N devices -> exit 2 with a message instead of a one-GPU number under an N-GPU label (the gloo rehearsal
    backend alone may stack ranks on one device)."""
    import socket
    import subprocess
    n = args.gpus
    ndev = torch.cuda.device_count()
    if ndev < n and args.dist_backend != "gloo":
        print(f"bench.py: --gpus {n} but this machine exposes {ndev} GPU(s): refusing to measure fewer ranks than asked "
              f"(use --dist-backend gloo for a control-flow rehearsal with several ranks on one GPU)", file=sys.stderr)
        return 2
    if ndev < 1:
        print("bench.py needs an MI355X (the HIP path has no CPU fallback)", file=sys.stderr)
        return 2
    port = os.environ.get("MASTER_PORT")
    if port is None:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = str(s.getsockname()[1])
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
                   OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n))))
        # rank 0 inherits stdout (it prints the ONE JSON line); the other ranks' stdout goes to stderr
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else sys.stderr))
    rc = 0
    alive = list(procs)
    try:
        while alive:
            time.sleep(0.2)
            for p in list(alive):
                code = p.poll()
                if code is None:
                    continue
                alive.remove(p)
                if code != 0:
                    rc = rc or code
                    print(f"bench.py launcher: rank {procs.index(p)} exited with code {code}; stopping the other ranks", file=sys.stderr)
                    for q in alive:         # exactly the children started above
                        q.terminate()
    finally:
        for q in alive:
            try:
                q.wait(timeout=20)
            except subprocess.TimeoutExpired:
                q.kill()
    return rc if rc >= 0 else 1


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    # stdout carries exactly ONE line (the JSON): native libraries print there too (RCCL writes a five-line version banner
    # to stdout when its first communicator comes up), so fd 1 points at stderr until the result is printed
    sys.stdout.flush()
    _stdout_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    assert torch.cuda.is_available(), "bench.py needs an MI355X (the HIP path has no CPU fallback)"
    ndev = torch.cuda.device_count()
    if world > ndev and args.dist_backend != "gloo":
        print(f"bench.py: WORLD_SIZE {world} but {ndev} GPU(s) visible: one rank per GPU or nothing", file=sys.stderr)
        sys.exit(2)
    local_rank = local_rank % max(ndev, 1)          # gloo rehearsal: several ranks may share one GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    train = args.mode == "train"
    dist_path = (world > 1 or args.rehearse_dist)
    if dist_path:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29655")
        if world == 1:
            torch.distributed.init_process_group(backend="nccl", rank=0, world_size=1, device_id=dev)
            from csts_amd import distributed as _du
            _du._FORCE = True        # 1-rank rehearsal: take the collective code paths anyway
        elif args.dist_backend == "gloo":
            torch.distributed.init_process_group(backend="gloo")
        else:
            torch.distributed.init_process_group(backend="nccl", device_id=dev)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE {world}"
    rccl_ranks = torch.distributed.get_world_size() if dist_path else 1

    from csts_amd.config import load_yaml
    from csts_amd.build import build_model
    from csts_amd import train as T
    from csts_amd import ops as _ops
    from csts_amd.distributed import GradAllReduce

    b, S = args.batch_per_gpu, args.crop
    opts = ["NUM_GPUS", min(world, ndev), "TRAIN.BATCH_SIZE", b * world, "MODEL.LOSS_FUNC", "kldiv+egonce", "MODEL.LOSS_ALPHA", 0.05,
            "DATA.NUM_FRAMES", args.frames, "CSTS_AMD.COMPUTE", args.compute]
    if args.trunk_cut is not None:
        opts += ["CSTS_AMD.TRUNK_CUT", args.trunk_cut]
    if args.bucket_dtype is None and args.compute != "fp32":
        # 16-bit compute modes: the gradient buckets travel in the same 16-bit type (half the xGMI bytes; the optimizer kernels
        # accumulate in fp32) -- stated in config.grad_bucket_dtype; --bucket-dtype fp32 restores the reference's fp32 all-reduce
        args.bucket_dtype = args.compute
    if args.bucket_dtype is not None:
        opts += ["CSTS_AMD.GRAD_BUCKET_DTYPE", args.bucket_dtype]
    if args.no_grad_factors:
        opts += ["CSTS_AMD.FUSION_GRAD_FACTORS", False]
    if args.one_stream:
        opts += ["CSTS_AMD.TWO_STREAMS", False]
    if S != 256:
        opts += ["DATA.TRAIN_CROP_SIZE", S, "DATA.TEST_CROP_SIZE", S, "CSTS_AMD.FUSION_KERNEL_FROM_GRID", True]
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"), opts)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg)
    core = model.module if isinstance(model, GradAllReduce) else model
    check = None
    if rank == 0 and args.full and not args.no_loss_check:
        check = loss_check(cfg, core, args.frames, b, S, dev, T)
    if train and dist_path and not isinstance(model, GradAllReduce):
        model = GradAllReduce(model, bucket_mb=cfg.CSTS_AMD.GRAD_BUCKET_MB)
    model.train(train)
    batch = T.synthetic_batch(b, args.frames, S, 1000 + rank, dev)      # resident in HBM before timing
    lr = T.get_lr_at_epoch(cfg, 0.0)
    step_kind = "eager"
    graphed = None
    if train:
        use_graph = not args.no_graph and not (dist_path and args.eager_dist)
        opt = T.construct_optimizer(model, cfg, capturable=use_graph)
        if use_graph and dist_path:
            # The graph chain has never run on more than one physical GPU.  If building it fails on ANY rank,
            # every rank falls back to the eager hook-driven step, so that a scaling run still produces its line.
            ok, why = 1, ""
            try:
                if os.environ.get("CSTS_BENCH_FAIL_CHAIN"):           # test hook for the fallback below
                    raise RuntimeError("forced by CSTS_BENCH_FAIL_CHAIN")
                graphed, step_kind = T.SegmentedTrainStep(cfg, model, opt, batch), "hip_graph_chain+eager_collectives"
            except Exception as e:                                    # noqa: BLE001 -- anything: the fallback is the point
                ok, why, graphed = 0, repr(e), None
                print(f"[bench] rank {rank}: graph chain failed ({why}); falling back to the eager data-parallel step", file=sys.stderr)
            flag = torch.tensor([ok], dtype=torch.int32, device=dev)
            if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                torch.cuda.synchronize()
                torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
            if int(flag.item()) == 0:
                graphed, step_kind = None, "eager+hook_buckets (graph chain unavailable)"
                if isinstance(model, GradAllReduce):
                    model.hooks_enabled = True
                    _ops.GROUP_WGRADS = "never"
                _ops.reset_deferred()
        elif use_graph:
            graphed, step_kind = T.GraphedTrainStep(cfg, model, opt, batch), "hip_graph"

        def step():
            if graphed is not None:
                return graphed.run(batch, lr)
            return T.train_step(cfg, model, batch, opt, lr)

        def eager_step():
            return T.train_step(cfg, model, batch, opt, lr)
    else:
        from csts_amd import losses

        def eager_step():
            with torch.no_grad():
                logits, v, a = core([batch["video"]], batch["audio"], return_embed=True)
                return losses.frame_softmax(logits, temperature=2), v, a
        fgraph = None
        if not args.no_graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    eager_step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            fgraph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(fgraph, capture_error_mode="thread_local"):
                fout = eager_step()
            step_kind = "hip_graph"

        def step():
            if fgraph is not None:
                fgraph.replay()
                return fout
            return eager_step()

    def sync():
        torch.cuda.synchronize()
        if dist_path:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    sync()
    dt = time.perf_counter() - t0
    if dist_path:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t)
    if args.dump_outputs and rank == 0:
        # now, before the steps below overwrite the graph's output buffers and update the weights again
        dump_outputs(args.dump_outputs, step_outputs(args.mode, res, core))
    clips = b * world * args.steps
    value = clips / dt
    ms_per_step = dt / args.steps * 1e3
    last_loss = float(res[0]) if train else None

    # ---- everything below up to the result line runs with --full only
    # ---- median of single steps by HIP events (>= 10 warm-up steps have run by now: warmup + the timed ones)
    median_ms = None
    if args.full:
        extra_warm = max(0, 10 - args.warmup - args.steps) if args.median_steps > 0 else 0
        for _ in range(extra_warm):
            step()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.median_steps + 1)]
        evs[0].record()
        for i in range(args.median_steps):
            step()
            evs[i + 1].record()
        torch.cuda.synchronize()
        per_step = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.median_steps)]
        median_ms = statistics.median(per_step) if per_step else None

    # ---- forward / loss / backward / optimizer split: the same step as a chain of graphs, each segment timed by events
    segments = None
    if args.full and train and world == 1 and not dist_path and not args.no_segments and not args.no_graph:
        try:
            seg = T.SegmentedTrainStep(cfg, model, opt, batch, warmup=1, trunk_cut=0)
            for _ in range(3):
                seg.run(batch, lr)
            rows = []
            for _ in range(15):
                seg.run(batch, lr, timed=True)
                rows.append(seg.segment_ms())
            med = [statistics.median(r[i] for r in rows) for i in range(5)]
            segments = {"fwd_ms": round(med[0], 3), "loss_ms": round(med[1], 3), "bwd_ms": round(med[2] + med[3], 3),
                        "bwd_head_ms": round(med[2], 3), "bwd_trunk_ms": round(med[3], 3), "optimizer_ms": round(med[4], 3),
                        "fwd_bwd_ms": round(med[0] + med[1] + med[2] + med[3], 3),
                        "note": "graph chain forward | eager losses | backward head | backward trunk | clip+AdamW, median of 15; "
                                "the headline step is ONE graph of the same kernels"}
            del seg
        except Exception as e:      # diagnostics only: never lose the headline line
            segments = {"error": repr(e)}

    roof = None
    if args.full and not args.no_roofline:
        # every rank runs the instrumented steps (they contain the gradient collectives); rank 0 reports its own timings
        _mode = _ops.GROUP_WGRADS
        if train and step_kind != "eager" and _mode == "capture":
            _ops.GROUP_WGRADS = "always"      # instrument the same kernel set the captured (timed) step runs
        if isinstance(model, GradAllReduce) and not model.hooks_enabled:
            model.hooks_enabled = True        # the instrumented eager steps reduce through the hook-driven buckets
            _ops.GROUP_WGRADS = "never"
        gt = GemmTimer()
        gt.install()
        two = core.two_streams
        core.two_streams = False        # one stream: an event pair then brackets exactly one kernel (plus its launch gap)
        # keep the launch stream ahead of the GPU: a spin kernel first, so that the host has every launch of the step
        # queued before the GPU reaches it and an event pair brackets the kernel alone, not the host's launch gap
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); torch.cuda._sleep(10_000_000); e1.record(); torch.cuda.synchronize()
        spin = int(10_000_000 * (120.0 if train else 40.0) / max(e0.elapsed_time(e1), 1e-3))     # head start
        for _ in range(2):
            torch.cuda._sleep(spin)
            eager_step()
        gt.remove()
        per_entry = None
        if train:
            # every C-ABI entry of one eager single-stream step with its algorithmic bytes / flop (tools/work_model.py)
            ot = OpTimer()
            ot.install()
            torch.cuda._sleep(spin)
            eager_step()
            t_ev0, t_ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ot.rec.clear()
            _ops.WG_STATS = []
            torch.cuda._sleep(spin)
            t_ev0.record()
            eager_step()
            t_ev1.record()
            ot.remove()
            extra = {}
            for entry, byt, fl in (_ops.WG_STATS or []):
                e = extra.setdefault(entry[5:], [0.0, 0.0])
                e[0] += byt
                e[1] += fl
            _ops.WG_STATS = None
            import work_model
            n_par = sum(p.numel() for p in core.parameters())
            n_sh = sum(l.weight.numel() for l in (getattr(core, "_w16_all", None) or []))
            fac = getattr(opt, "_factored", None) or []       # fusion convs updated from their gradient factors (csts_adamw_factored)
            n_fac = sum(opt.params[i].numel() for i, _, _ in fac)
            n_fac_sh = sum(opt.params[i].numel() for i, _, _ in fac if i in getattr(opt, "_shadow_by_index", {}))
            extra["adamw_step"] = work_model.work_adamw(n_par - n_fac, n_sh - n_fac_sh)
            if fac:
                fbytes = sum(dy.numel() * dy.element_size() + a_.numel() * a_.element_size() for _, dy, a_ in fac)
                extra["adamw_factored"] = (n_fac * 24 + n_fac_sh * 2 + fbytes, sum(2.0 * dy.shape[0] * opt.params[i].numel() for i, dy, _ in fac))
                extra["factored_sqnorm"] = (fbytes, sum(2.0 * dy.shape[0] * dy.shape[0] * (dy.shape[1] + a_.shape[1]) for _, dy, a_ in fac))
            ops_ms = per_entry = ot.summary(1, extra)
            tot = t_ev0.elapsed_time(t_ev1)
            if args.op_breakdown:
                with open(args.op_breakdown if rank == 0 else os.devnull, "w") as f:
                    f.write(f"single-stream eager step {tot:.2f} ms; C-ABI kernels {sum(v['ms'] for v in ops_ms.values()):.2f} ms; "
                            f"torch-native remainder (autograd adds, casts, fills) {tot - sum(v['ms'] for v in ops_ms.values()):.2f} ms\n")
                    f.write("entry                        calls        ms   algorithmic MB   GFLOP   hbm_frac(8 TB/s)  mfma_frac(2.5 PF)\n")
                    for k, v in ops_ms.items():
                        f.write(f"{k:28s} {v['calls']:5d} calls {v['ms']:8.3f} ms" + (
                            f"  {v['algorithmic_bytes'] / 1e6:10.1f} MB {v['algorithmic_flop'] / 1e9:9.1f}  {v['hbm_frac']:8.3f} {v['mfma_frac']:8.3f}  {v['bound']}"
                            if "hbm_frac" in v else "") + "\n")
        core.two_streams = two
        _ops.GROUP_WGRADS = _mode
        agg = gt.summary()
        if args.dump_gemm and rank == 0:
            gt.dump_shapes(args.dump_gemm)
        if args.dump_gemm_order and rank == 0:
            gt.dump_order(args.dump_gemm_order, 2)
        # dominant kernel = the single-kernel GEMM variant (no split-K finishing pass inside the event pair) with the most time
        single = {k: v for k, v in agg.items() if not v[4]}
        name = max(single, key=lambda k: single[k][3]) if single else None
        n, fl, by, sec, _, ext = agg.get(name, (0, 0.0, 0.0, 1.0, False, 0.0))
        sec_eager, timing = sec, "HIP events around each launch of an eager single-stream pass"
        replay = None
        if name is not None and step_kind != "eager" and torch.cuda.is_available():
            # `value` is measured on a graph replay: time the dominant kernel's launches the same way (the eager event pairs
            # above also bracket the event-record packets and read ~10 % high: profiles/r3_gemm_replay_shapes.txt)
            try:
                nl, t_med, t_min = gt.replay_kernel(name, 2)
                if nl and nl == n // 2:
                    replay = {"launches": nl, "avg_launch_us_median_replay": round(t_med / nl * 1e6, 2), "avg_launch_us_best_replay": round(t_min / nl * 1e6, 2),
                              "avg_launch_us_eager_events": round(sec_eager / max(n, 1) * 1e6, 2)}
                    sec = t_med * 2            # fl / by / n cover the two instrumented steps
                    timing = ("HIP events around a HIP-graph replay of this kernel's launches of one step (same shapes / leading dimensions / "
                              "epilogues, step order, scratch operands rotating over 3 sets per shape), median of 6 replays")
            except Exception as e:      # diagnostics: keep the eager figure
                replay = {"error": repr(e)}
        tot_sec = sum(a[3] for a in agg.values())
        tot_fl = sum(a[1] for a in agg.values())
        peak = PEAK_BF16_TFLOPS if args.compute in ("bf16", "fp16") else 157.3      # dense f16 MFMA rate == bf16 rate on gfx950
        traffic, traffic_src = None, "profiles/pmc_traffic.json: no entry for this kernel"
        try:     # HBM bytes per launch from the rocprofv3 --pmc passes (tools/pmc_traffic.py), same command, same kernel
            pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import build_stamp
            cur, st = build_stamp.current(), pmc.get("stamp")
            key = "lib_f16_sha256" if args.compute == "fp16" else "lib_sha256"
            ent = pmc["kernels"].get(name)
            if st is None:
                traffic_src = "profiles/pmc_traffic.json carries no build stamp (collected before round 5): traffic withheld"
            elif st.get(key) != cur.get(key):
                traffic_src = (f"profiles/pmc_traffic.json was collected on another build of the library (stamp {str(st.get(key))[:12]}, "
                               f"running {str(cur.get(key))[:12]}): traffic withheld")
            elif ent is None:
                pass
            elif ent.get("launches_per_step") is not None and int(round(ent["launches_per_step"])) != n // 2:
                traffic_src = (f"profiles/pmc_traffic.json profiled {ent['launches_per_step']:g} launches of this kernel per step, this run "
                               f"timed {n // 2}: another population, traffic withheld")
            else:
                traffic = ent["hbm_bytes_per_launch"]
                traffic_src = (f"profiles/pmc_traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command (FETCH_SIZE doubled, "
                               f"gfx950), {ent.get('launches_per_step', '?'):g} launches per step, library sha256 {str(st.get(key))[:16]}, "
                               f"source commit {str(st.get('source_commit'))[:12]}{'+dirty' if st.get('source_dirty') else ''}")
        except Exception as e:
            traffic_src = f"profiles/pmc_traffic.json unreadable ({e!r})"
        # the binding roofline of this kernel: t_min = max(flops / P_mfma, algorithmic bytes / P_hbm)
        t_mfma, t_hbm = fl / (peak * 1e12), by / (PEAK_HBM_GBS * 1e9)
        hbm_bound = t_hbm > t_mfma
        roof = {"bound": "hbm" if hbm_bound else "mfma", "kernel": name,
                "achieved": round(by / sec / 1e9, 1) if hbm_bound else round(fl / sec / 1e12, 2),
                "peak": PEAK_HBM_GBS if hbm_bound else peak, "unit": "GB/s" if hbm_bound else "TFLOP/s",
                "frac": round(max(t_mfma, t_hbm) / sec, 4),
                "mfma_tflops": round(fl / sec / 1e12, 2), "mfma_frac": round(t_mfma / sec, 4),
                "algorithmic_gbps": round(by / sec / 1e9, 1), "hbm_frac": round(t_hbm / sec, 4),
                "traffic": traffic, "traffic_source": traffic_src,
                "launches_per_step": n // 2, "avg_launch_us": round(sec / max(n, 1) * 1e6, 2), "timing": timing, "graph_replay": replay,
                "algorithmic_flop_per_launch": round(fl / max(n, 1)), "algorithmic_bytes_per_launch": round(by / max(n, 1)),
                "epilogue_operand_bytes_per_launch": round(ext / max(n, 1)),     # GELU pre-activation out / in, residual in: on top of A + B + C
                "hbm_frac_incl_epilogue_operands": round((by + ext) / (PEAK_HBM_GBS * 1e9) / sec, 4),
                "all_gemm_tflops": round(tot_fl / tot_sec / 1e12, 2), "all_gemm_ms_per_step": round(tot_sec / 2 * 1e3, 2),
                "per_kernel": {k: {"launches_per_step": v[0] // 2, "avg_us": round(v[3] / v[0] * 1e6, 1),
                                   "tflops": round(v[1] / v[3] / 1e12, 1), "ms_per_step": round(v[3] / 2 * 1e3, 3)}
                               for k, v in sorted(agg.items(), key=lambda kv: -kv[1][3])[:8]}}
        if per_entry is not None:
            # every C-ABI entry point of one step (non-GEMM kernels included): calls, eager-event ms, algorithmic bytes / flop
            # (tools/work_model.py: every operand once) and the roofline fractions they give
            roof["per_entry"] = {k: v for k, v in list(per_entry.items())[:24]}
            roof["per_entry_note"] = ("HIP events around each C-ABI call of one eager single-stream step (8-12 % above the graph replay); "
                                      "hbm_frac = algorithmic bytes / ms / 8 TB/s, mfma_frac = algorithmic flop / ms / 2.5 PF")
    if dist_path:
        torch.distributed.barrier()

    rc = 0
    if rank == 0:
        per_gpu = value / world
        mult = 3 if train else 1
        gflop = mult * FWD_GFLOP_PER_CLIP.get(args.frames, 0.0) * (S / 256.0) ** 2
        gb = mult * BYTES_FWD_GB_PER_CLIP.get(args.frames, 0.0) * (S / 256.0) ** 2
        what = ("train step (fwd + KLDiv + 0.05*EgoNCE + bwd" + (" + RCCL grad all-reduce" if dist_path else "") + " + clip + AdamW)") \
            if train else "eval forward + frame_softmax"
        out = {
            "metric": f"clips/sec {'training (fwd+bwd)' if train else 'forward'} CSTS-Ego4D {args.frames}x{S}^2 {args.compute}",
            "value": round(value, 3), "unit": "clips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.compute, "data": "synthetic",
            "config": {"workload": f"CSTS_Ego4D_Gaze_Forecast.yaml {what}, {args.frames}x{S}^2 video + 24 kHz STFT audio, b={b}/GPU",
                       "mode": args.mode, "global_batch": b * world, "frames": args.frames, "crop": S, "parallelism": f"dp{world}",
                       "step": step_kind, "hip_graph": step_kind != "eager", "rccl_ranks": rccl_ranks,
                       **({"trunk_cut": int(graphed.trunk_cut)} if hasattr(graphed, "trunk_cut") else {}),
                       **({"grad_bucket_dtype": ("16-bit" if graphed.bucket16 else "fp32")} if hasattr(graphed, "bucket16") else {}),
                       **({"fusion_grad_factors": bool(graphed.factor_params),
                           "allreduce_mb_per_step": round(sum((f[0].numel() - (sum((p.numel() + 3) // 4 * 4 for p in graphed.factor_params) if k == 0 else 0))
                                                               * f[0].element_size() for k, f in enumerate(graphed.flat16 if graphed.bucket16 else graphed.flat)) / 1e6, 1)}
                          if (hasattr(graphed, "factor_params") and getattr(graphed, "dist", False)) else {}),
                       "dist_backend": (torch.distributed.get_backend() if dist_path else None),
                       "note": ("256^2 not 224^2: the reference's (1,8,8) fusion convs reject 224^2 (SURVEY.md D1)" if S == 256 else
                                "EXTENSION, parity unpinned: 224^2 with (1,7,7) fusion kernels (CSTS_AMD.FUSION_KERNEL_FROM_GRID); "
                                "the reference cannot run this grid, FLOP/byte figures scaled by (224/256)^2")},
            **({"median_step_ms": round(median_ms, 3) if median_ms is not None else None,
                "median_over_steps": args.median_steps,
                "median_clips_per_s": round(b * world / median_ms * 1e3, 3) if median_ms else None} if args.full else {}),
            "end_to_end_roofline": {"mfma_frac": round(per_gpu * gflop / 1e3 / PEAK_BF16_TFLOPS, 4),
                                    "hbm_frac": round(per_gpu * gb / PEAK_HBM_GBS, 4),
                                    "gflop_per_clip": round(gflop, 1), "gb_per_clip": round(gb, 2)},
        }
        if last_loss is not None:
            out["loss"] = round(last_loss, 5)
        if segments is not None:
            out["segments"] = segments
            for k in ("fwd_bwd_ms", "optimizer_ms"):
                if k in segments:
                    out[k] = segments[k]
        if check is not None:
            out["loss_check"] = check
            if check.get("status") == "MISMATCH":
                rc = 3
        if roof is not None:
            out["roofline"] = roof
        if args.full and world == 1 and not dist_path and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args.frames, args.mode, args.quick_cpu_baseline, batch=args.batch_per_gpu)
            except Exception as e:  # keep the line valid even if the host runs out of memory
                out["cpu_baseline"] = {"value": None, "error": repr(e)}
        sys.stdout.flush()
        os.dup2(_stdout_fd, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)       # teardown chatter of native libraries stays off stdout as well
        if rc:
            print(f"bench.py: loss check FAILED: {check}", file=sys.stderr)
    if dist_path:
        torch.distributed.destroy_process_group()
    sys.exit(rc)


if __name__ == "__main__":
    main()
