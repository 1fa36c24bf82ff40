#!/usr/bin/env python3
"""Write tests/golden/gaze_meters.npz by RUNNING THE REFERENCE's gaze meters.

Build-container tooling only (needs the reference checkout; never runs on the GPU box, never imported by the product):

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_meters.py --reference DIR     (DIR: a checkout of the reference)

slowfast/utils/meters.py and metrics.py are imported unmodified from the reference behind import-only stubs
(fvcore.common.timer, slowfast.utils.logging whose log_json_stats records the dict it is given, slowfast.utils.misc).  One
seeded sequence of batches (small 16 x 16 maps) is driven through TrainGazeMeter, ValGazeMeter and TestGazeMeter the way the
three reference loops do (tools/train_avgaze_net.py:124-155,196-217, tools/test_avgaze_net.py:68-92): min-max rescale,
adaptive_f1, update_stats, log_iter_stats, and log_epoch_stats / finalize_metrics at the end -- once per threshold table.
torch.argmax is wrapped only to RECORD the f1 vector it is given, from which the generator asserts that no best threshold is a
near-tie.  Stored: the inputs, the per-batch adaptive_f1 results, the window medians of the meters' ScalarMeters after every
batch, and every logged record."""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gaze_meters.npz")
DATASETS = ["ego4d_av_gaze_forecast", "aria_av_gaze_forecast", "ego4d_av_gaze"]     # the three threshold tables, fixation type 0
NB, B, T, S = 12, 2, 4, 16        # batches, clips per batch, frames per clip, map side
WINDOW = 5                        # cfg.LOG_PERIOD: log points after batches 5 and 10, the second one on a wrapped window
NO_WEIGHT_BATCH = 3               # this batch has no frame of gaze type 1: ValGazeMeter / TestGazeMeter give it weight 0
MIN_GAP = 1e-4
SEED = 20261020                   # the first of a few seeds tried whose sequence meets every condition asserted in main()
LOGGED = []


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Timer:
    def reset(self):
        pass

    def pause(self):
        pass

    def seconds(self):
        return 0.0


class _Logger:
    def info(self, *a, **k):
        pass


def import_reference(ref_root):
    """slowfast.utils.{meters, metrics} from the reference tree without running the packages' __init__."""
    _mod("fvcore")
    _mod("fvcore.common")
    _mod("fvcore.common.timer", Timer=_Timer)
    pkg = os.path.join(ref_root, "slowfast")
    _mod("slowfast", __path__=[pkg])
    _mod("slowfast.utils", __path__=[os.path.join(pkg, "utils")])
    _mod("slowfast.utils.logging", log_json_stats=lambda stats: LOGGED.append(dict(stats)), get_logger=lambda name: _Logger())
    _mod("slowfast.utils.misc", gpu_mem_usage=lambda: 0.0, cpu_mem_usage=lambda: (0.0, 0.0))
    metrics = importlib.import_module("slowfast.utils.metrics")
    meters = importlib.import_module("slowfast.utils.meters")
    return meters, metrics


class RecordF1:
    """torch.argmax wrapped to keep the vector adaptive_f1 takes its maximum of (metrics.py:71)."""

    def __enter__(self):
        self.real = torch.argmax
        self.seen = []

        def argmax(x, *a, **k):
            self.seen.append(x.detach().clone())
            return self.real(x, *a, **k)
        torch.argmax = argmax
        return self

    def __exit__(self, *exc):
        torch.argmax = self.real


def gap_of(f1):
    top = torch.sort(f1.double(), descending=True)[0]
    return float(top[0] - top[1])


def rescale(preds):
    """tools/train_avgaze_net.py:125-127, the expression all three loops apply before adaptive_f1."""
    p = preds.detach().view(preds.size()[:-2] + (preds.size(-1) * preds.size(-2),))
    p = (p - p.min(dim=-1, keepdim=True)[0]) / (p.max(dim=-1, keepdim=True)[0] - p.min(dim=-1, keepdim=True)[0] + 1e-6)
    return p.view(preds.size())


def make_batch(rng, types):
    """Softmaxed heat maps with a bump near the gaze point over log-normal clutter, so that after the min-max rescale the
    clutter straddles every threshold table; 5 x 5-ish Gaussian label maps; labels (x, y, gaze type)."""
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    xy = rng.uniform(0.15, 0.85, (B, T, 2))
    miss = rng.normal(0.0, 1.2, (B, T, 2))
    preds = np.empty((B, 1, T, S, S), dtype=np.float32)
    hm = np.empty((B, T, S, S), dtype=np.float32)
    for b in range(B):
        for t in range(T):
            cx, cy = xy[b, t] * (S - 1)
            k = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 1.5 ** 2))
            hm[b, t] = k / k.sum()
            px, py = cx + miss[b, t, 0], cy + miss[b, t, 1]
            logit = 4.5 * np.exp(-((xx - px) ** 2 + (yy - py) ** 2) / (2 * 2.0 ** 2)) + rng.normal(0.0, 0.9, (S, S))
            e = np.exp(logit - logit.max())
            preds[b, 0, t] = e / e.sum()
    labels = np.concatenate([xy, types.reshape(B, T, 1).astype(np.float64)], axis=-1)
    return torch.from_numpy(preds), torch.from_numpy(hm), torch.from_numpy(labels)


def make_types(rng, bi):
    while True:
        ty = rng.integers(0, 3, B * T)
        if bi == NO_WEIGHT_BATCH:
            ty[ty == 1] = 2
        if (ty == 0).sum() >= 2 and (bi == NO_WEIGHT_BATCH or (ty == 1).any()):
            return ty


def cfg_stub():
    return types.SimpleNamespace(LOG_PERIOD=WINDOW, OUTPUT_DIR=".", NUM_GPUS=1, SOLVER=types.SimpleNamespace(MAX_EPOCH=1))


def plain(rec):
    return {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in rec.items()
            if k in ("_type", "split", "iter", "f1", "recall", "precision", "threshold")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CSTS_REFERENCE"), help="checkout of the reference repository")
    ap.add_argument("--seed", type=int, default=SEED, help="seed of the batch sequence (the conditions on it are asserted)")
    args = ap.parse_args()
    if not args.reference or not os.path.isfile(os.path.join(args.reference, "slowfast", "utils", "meters.py")):
        ap.error("--reference DIR (or CSTS_REFERENCE) must name a checkout of the reference repository")
    meters, metrics = import_reference(args.reference)
    rng = np.random.default_rng(args.seed)
    batches = [make_batch(rng, make_types(rng, bi)) for bi in range(NB)]
    all_types = np.concatenate([b[2][..., 2].numpy().ravel() for b in batches])
    assert NB >= 7 and set(all_types.tolist()) == {0.0, 1.0, 2.0}
    assert not (batches[NO_WEIGHT_BATCH][2][..., 2] == 1).any()
    assert all((b[2][..., 2] == 0).any() for b in batches)
    arrays = {"preds": torch.stack([b[0] for b in batches]).numpy(), "labels_hm": torch.stack([b[1] for b in batches]).numpy(),
              "labels": torch.stack([b[2] for b in batches]).numpy()}
    meta = {"datasets": DATASETS, "window": WINDOW, "no_weight_batch": NO_WEIGHT_BATCH, "min_gap": MIN_GAP}
    for di, dataset in enumerate(DATASETS):
        cfg = cfg_stub()
        train = meters.TrainGazeMeter(NB, cfg)
        val = meters.ValGazeMeter(NB, cfg)
        test = meters.TestGazeMeter(NB * B, 1, 1, NB, dataset)
        per_batch, med_train, med_val, gaps = [], [], [], []
        del LOGGED[:]
        for it, (preds, labels_hm, labels) in enumerate(batches):
            pr = rescale(preds)
            with RecordF1() as rec:
                f1, recall, precision, threshold = metrics.adaptive_f1(pr, labels_hm, labels, dataset=dataset)
            gaps.append(gap_of(rec.seen[0]))
            per_batch.append([f1, recall, precision, threshold])
            train.update_stats(f1, recall, precision, threshold, 0.0, 0.0, mb_size=preds.size(0) * max(cfg.NUM_GPUS, 1))
            train.iter_toc()
            train.log_iter_stats(0, it)
            train.iter_tic()
            val.iter_toc()
            val.update_stats(f1, recall, precision, labels, threshold)
            val.log_iter_stats(0, it)
            val.iter_tic()
            test.iter_toc()
            test.update_stats(f1, recall, precision, preds=pr, labels_hm=labels_hm, labels=labels)
            test.iter_tic()
            med_train.append([train.f1.get_win_median(), train.recall.get_win_median(), train.precision.get_win_median(), train.threshold])
            med_val.append([val.f1.get_win_median(), val.recall.get_win_median(), val.precision.get_win_median(), val.threshold])
        train.log_epoch_stats(0)
        val.log_epoch_stats(0)
        with RecordF1() as rec:
            test.finalize_metrics()
        gaps.append(gap_of(rec.seen[0]))
        assert min(gaps) > MIN_GAP, (dataset, gaps)
        assert np.isfinite(np.array(per_batch)).all()
        logged = [plain(r) for r in LOGGED]
        kinds = [r.get("_type", r.get("split")) for r in logged]
        assert kinds == ["train_iter", "val_iter"] * (NB // WINDOW) + ["train_epoch", "val_epoch", "test_final"], kinds
        p = f"d{di}_"
        arrays.update({p + "per_batch": np.array(per_batch, dtype=np.float64), p + "median_train": np.array(med_train, dtype=np.float64),
                       p + "median_val": np.array(med_val, dtype=np.float64), p + "gaps": np.array(gaps),
                       p + "logged": np.array(json.dumps(logged))})
        print(f"{dataset:24s} smallest f1 gap {min(gaps):.2e}; test_final {logged[-1]}")
    # the NaN rule alone: a batch without a frame of the fixation type (kept out of the meter sequences: it would poison them)
    preds, labels_hm, labels = make_batch(rng, np.array([1, 2] * (B * T // 2)))
    res = metrics.adaptive_f1(rescale(preds), labels_hm, labels, dataset=DATASETS[0])
    assert all(np.isnan(v) for v in res[:3])
    arrays.update({"nan_preds": preds.numpy(), "nan_labels_hm": labels_hm.numpy(), "nan_labels": labels.numpy(),
                   "nan_result": np.array(res[:3], dtype=np.float64)})
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.0f} kB")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
