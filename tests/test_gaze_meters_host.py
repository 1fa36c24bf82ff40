"""Gaze meters, host side (no GPU): the library's meter rule (csts_gaze_meter_update_host, the function the device kernel
runs) fed per-frame counts formed with numpy from the frames of tests/golden/gaze_meters.npz reproduces what the reference's
TrainGazeMeter / ValGazeMeter / TestGazeMeter logged for the same batches (tools/gen_golden_meters.py ran them): window
medians after every batch and at the log points, epoch statistics, and the data-set-level adaptive F1 of finalize_metrics.

Tolerance against the reference: 2e-6 absolute on f1 / recall / precision (values in [0, 1], fp32 means in the reference; the
bound test_adaptive_f1_on_device uses for the same quantities); thresholds equal to 1e-12."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "gaze_meters.npz")
TOL, TOL_THR = 2e-6, 1e-12
NEW_SYMBOLS = ("csts_f1_counts", "csts_gaze_meter_state_bytes", "csts_gaze_meter_reset", "csts_gaze_meter_update",
               "csts_gaze_meter_update_host")


def load_fixture():
    z = np.load(FIXTURE)
    meta = json.loads(str(z["meta"]))
    return z, meta


def counts_of(preds, labels_hm, thresholds):
    """What f1_count_kernel writes, with numpy: per frame tp and fg_preds per threshold and fg_labels, after the fp32 min-max
    rescale of train_avgaze_net.py:125-127."""
    p = preds.astype(np.float32).reshape(-1, preds.shape[-2] * preds.shape[-1])
    q = labels_hm.astype(np.float32).reshape(p.shape)
    mn, mx = p.min(axis=1, keepdims=True), p.max(axis=1, keepdims=True)
    v = (p - mn) / (mx - mn + np.float32(1e-6))
    lab = q > np.float32(0.001)
    thr = thresholds.astype(np.float32)
    pr = v[:, None, :] > thr[None, :, None]
    tp = (pr & lab[:, None, :]).sum(-1)
    return np.concatenate([tp, pr.sum(-1), lab.sum(-1, keepdims=True)], axis=1).astype(np.int32)


def datasets():
    _, meta = load_fixture()
    return list(enumerate(meta["datasets"]))


def feed(meter, z, dataset, batches=None, chunks=None, after=None):
    """Batches of the fixture into a host meter; ``chunks`` regroups the same clips into other batch sizes; ``after(i)`` runs
    after the i-th update."""
    from csts_amd import metrics
    thr = metrics.thresholds_for(dataset)
    preds, hm, labels = z["preds"], z["labels_hm"], z["labels"]
    if chunks is not None:
        preds, hm, labels = (a.reshape((-1,) + a.shape[2:]) for a in (preds, hm, labels))
        edges = np.cumsum([0] + list(chunks))
        assert edges[-1] == preds.shape[0]
        groups = [slice(a, b) for a, b in zip(edges[:-1], edges[1:])]
    else:
        groups = list(range(preds.shape[0])) if batches is None else list(batches)
    for i, g in enumerate(groups):
        meter.update_counts(counts_of(preds[g], hm[g], thr), labels[g], batch_size=preds[g].shape[0])
        if after is not None:
            after(i)


def close(got, want, keys=("f1", "recall", "precision")):
    for k in keys:
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])


@pytest.mark.parametrize("di,dataset", datasets())
def test_window_medians_and_epoch_stats_equal_the_reference_meters(di, dataset):
    from csts_amd import metrics
    z, meta = load_fixture()
    logged = json.loads(str(z[f"d{di}_logged"]))
    for mode, med_key in (("train", "median_train"), ("val", "median_val")):
        m = metrics.HostGazeMeter(dataset, meta["window"], mode)
        med = z[f"d{di}_{med_key}"]
        per_batch = z[f"d{di}_per_batch"]
        log_points = []

        def after(i):
            got = m.window_median()
            assert np.abs(np.array([got["f1"], got["recall"], got["precision"]]) - med[i, :3]).max() <= TOL
            assert abs(got["threshold"] - med[i, 3]) <= TOL_THR
            last = m.last_batch()
            assert np.abs(np.array(last[:3]) - per_batch[i, :3]).max() <= TOL and abs(last[3] - per_batch[i, 3]) <= TOL_THR
            if (i + 1) % meta["window"] == 0:              # log_iter_stats speaks every LOG_PERIOD iterations
                rec = [r for r in logged if r.get("_type") == f"{mode}_iter" and r["iter"] == f"{i + 1}/{len(med)}"]
                assert len(rec) == 1
                close(got, rec[0])
                assert abs(got["threshold"] - rec[0]["threshold"]) <= TOL_THR
                log_points.append(i + 1)

        feed(m, z, dataset, after=after)
        assert len(log_points) == 2
        assert m.iterations() == len(med) > meta["window"]            # the ring wrapped
        epoch = [r for r in logged if r.get("_type") == f"{mode}_epoch"]
        assert len(epoch) == 1
        close(m.epoch_stats(), epoch[0])


@pytest.mark.parametrize("di,dataset", datasets())
def test_dataset_stats_equal_finalize_metrics_for_any_chunking(di, dataset):
    from csts_amd import metrics
    z, meta = load_fixture()
    final = [r for r in json.loads(str(z[f"d{di}_logged"])) if r.get("split") == "test_final"]
    assert len(final) == 1
    nclips = z["preds"].shape[0] * z["preds"].shape[1]
    results = []
    for chunks in (None, [5, 1, 7, nclips - 13], [nclips]):
        m = metrics.HostGazeMeter(dataset, meta["window"], "test")
        feed(m, z, dataset, chunks=chunks)
        got = m.dataset_stats()
        close(got, final[0])
        assert abs(got["threshold"] - final[0]["threshold"]) <= TOL_THR
        results.append(got)
    assert results[0]["frames"] == results[1]["frames"] == results[2]["frames"] == int((z["labels"][..., 2] == 0).sum())
    for r in results[1:]:          # the sums are fp64 over the same frames in the same order, split at other places
        assert all(abs(r[k] - results[0][k]) <= 1e-12 for k in ("f1", "recall", "precision")) and r["threshold"] == results[0]["threshold"]


def test_zero_weight_batch_changes_no_epoch_total_and_reset_clears():
    from csts_amd import metrics
    z, meta = load_fixture()
    dataset, k = meta["datasets"][0], meta["no_weight_batch"]
    assert not (z["labels"][k][..., 2] == 1).any() and (z["labels"][k][..., 2] == 0).any()
    m = metrics.HostGazeMeter(dataset, meta["window"], "val")
    feed(m, z, dataset, batches=range(k))
    before, frames = m.epoch_stats(), m.dataset_stats()["frames"]
    feed(m, z, dataset, batches=[k])
    assert m.epoch_stats() == before and m.iterations() == k + 1
    assert m.dataset_stats()["frames"] == frames + int((z["labels"][k][..., 2] == 0).sum())      # still counted in the data-set sums
    # the train meter weighs the same batch with its clip count
    t = metrics.HostGazeMeter(dataset, meta["window"], "train")
    feed(t, z, dataset, batches=[k])
    assert t.epoch_stats()["samples"] == z["preds"].shape[1]
    m.reset()
    assert not m.state.any() and m.iterations() == 0
    assert all(np.isnan(m.epoch_stats()[key]) for key in ("f1", "recall", "precision"))       # zero samples: NaN, no exception
    assert np.isnan(m.dataset_stats()["f1"])
    with pytest.raises(ValueError):
        m.window_median()


def test_batch_without_a_fixation_frame_gives_nan():
    from csts_amd import metrics
    z, meta = load_fixture()
    dataset = meta["datasets"][0]
    assert np.isnan(z["nan_result"]).all() and not (z["nan_labels"][..., 2] == 0).any()
    m = metrics.HostGazeMeter(dataset, meta["window"], "val")
    m.update_counts(counts_of(z["nan_preds"], z["nan_labels_hm"], metrics.thresholds_for(dataset)), z["nan_labels"])
    assert all(np.isnan(v) for v in m.last_batch()[:3])
    assert m.dataset_stats()["frames"] == 0


def test_fixture_meets_the_conditions_it_was_generated_under():
    z, meta = load_fixture()
    ty = z["labels"][..., 2]
    assert z["preds"].shape[0] >= 7 and meta["window"] == 5
    assert set(np.unique(ty).tolist()) == {0.0, 1.0, 2.0}
    assert all((ty[b] == 0).any() for b in range(ty.shape[0]))
    assert sum(not (ty[b] == 1).any() for b in range(ty.shape[0])) >= 1
    assert len(meta["datasets"]) == 3
    for di in range(3):
        assert z[f"d{di}_gaps"].min() > 1e-4 and len(z[f"d{di}_gaps"]) == ty.shape[0] + 1
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_bad_arguments_are_rejected():
    from csts_amd import lib as L, metrics
    lib = L.load()
    assert lib.csts_gaze_meter_state_bytes(0, 5) == 0 and lib.csts_gaze_meter_state_bytes(65, 5) == 0
    assert lib.csts_gaze_meter_state_bytes(31, 5) == (5 + 62) * 8 + 5 * 16
    state = np.zeros(64, dtype=np.int64)
    counts = np.zeros((2, 7), dtype=np.int32)
    lab = np.zeros((2, 3))
    assert lib.csts_gaze_meter_update_host(counts.ctypes.data, lab.ctypes.data + 16, 3, 2, 65, 0, 1, -1, 5, state.ctypes.data) != 0
    assert lib.csts_gaze_meter_update_host(counts.ctypes.data, lab.ctypes.data + 16, 3, 2, 3, 0, 1, -1, 0, state.ctypes.data) != 0
    assert lib.csts_gaze_meter_update_host(None, lab.ctypes.data + 16, 3, 2, 3, 0, 1, -1, 5, state.ctypes.data) != 0
    assert b"null pointer" in lib.csts_last_error()
    with pytest.raises(ValueError):
        metrics.HostGazeMeter("ego4d_av_gaze", 5, "eval")
    with pytest.raises(NotImplementedError):
        metrics.HostGazeMeter("kinetics", 5, "val")
    with pytest.raises(ValueError):
        metrics.HostGazeMeter("ego4d_av_gaze", 5, "train").update_counts(np.zeros((2, 23), dtype=np.int32), lab)


def test_header_binding_and_both_libraries_agree_on_the_new_names():
    from csts_amd import lib as L
    header = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in L.SYMBOLS
    L.load()        # raises if libcsts_hip.so lacks any of lib.SYMBOLS
    code = "from csts_amd import lib; lib.set_half('fp16'); h = lib.load(); " + \
           "; ".join(f"assert h.{n}" for n in NEW_SYMBOLS) + "; print('ok')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]


def test_config_keys_default_off():
    from csts_amd.config import get_cfg
    cfg = get_cfg()
    assert cfg.CSTS_AMD.GAZE_METERS is False and cfg.CSTS_AMD.TEST_STEPS == 1
