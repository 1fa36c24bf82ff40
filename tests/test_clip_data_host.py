"""Host side of the recorded-clip path (no GPU): csts_amd.datasets.clip_rule against infer.plan_video (val / test) and against
the label frames of ego4d_avgaze_forecast.py:230-235 / aria_avgaze_forecast.py:226-231 written out (train), the replacement of
clips whose label rows run out, the epoch sampler plan_epoch, the label columns of the two datasets, and the three entry points
of csts_amd/csrc/batch.hip in both kernel libraries."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from csts_amd import datasets as D  # noqa: E402
from csts_amd import inputs, lib  # noqa: E402
from csts_amd.config import assert_and_infer_cfg, load_yaml  # noqa: E402
from csts_amd.infer import plan_video  # noqa: E402

EGO = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ARIA = os.path.join(ROOT, "configs/Aria/CSTS_Aria_Gaze_Forecast.yaml")
CASES = [(EGO, 150, 1001, 86), (ARIA, 100, 801, 60)]
# labels_idx of the cited lines, T = 8: ego4d linspace(last + 1, last + 150 - 86, 8), aria linspace(last + 1 + 4, last + 100 - 60, 8)
TRAIN_LABEL_ROWS = {
    (EGO, 0.0): [64, 73, 82, 91, 100, 109, 118, 127],          # last input frame 63
    (EGO, 0.999): [85, 94, 103, 112, 121, 130, 139, 148],      # last input frame 84
    (ARIA, 0.0): [40, 45, 50, 55, 60, 65, 70, 75],             # last input frame 35, + SAMPLING_RATE 4
    (ARIA, 0.999): [63, 68, 73, 78, 83, 88, 93, 98],           # last input frame 58
}


@pytest.mark.parametrize("yaml,n_frames,cols,observed", CASES)
@pytest.mark.parametrize("mode", ["val", "test"])
def test_clip_rule_eval_is_window_0_of_plan_video(yaml, n_frames, cols, observed, mode):
    cfg = load_yaml(yaml)
    r = D.clip_rule(cfg, mode, n_frames, cols)
    plan = plan_video(cfg, n_frames, cols=cols)
    assert np.array_equal(r["frames"], plan["frames_idx"][0])
    assert np.array_equal(r["label_rows"], plan["target_idx"][0])
    assert np.array_equal(r["centers"], plan["audio_centers"][0])
    assert r["observed"] == observed == plan["observed"] and r["usable"] == observed * cols // n_frames


@pytest.mark.parametrize("yaml,n_frames,cols,observed", CASES)
@pytest.mark.parametrize("u", [0.0, 0.999])
def test_clip_rule_train(yaml, n_frames, cols, observed, u):
    cfg = load_yaml(yaml)
    r = D.clip_rule(cfg, "train", n_frames, cols, u=u)
    _, _, want = inputs.temporal_indices(observed, cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, -1, cfg.TEST.NUM_ENSEMBLE_VIEWS, u=u)
    assert np.array_equal(r["frames"], want) and r["frames"].dtype == np.int64
    assert r["label_rows"].tolist() == TRAIN_LABEL_ROWS[(yaml, u)]
    assert int(r["frames"][-1]) == TRAIN_LABEL_ROWS[(yaml, u)][0] - 1 - (cfg.DATA.SAMPLING_RATE if yaml == ARIA else 0)
    # the audio centres: round(frame / observed * usable), kept 128 columns inside the trimmed spectrogram (:215-218)
    usable = int(cols * observed / n_frames)
    assert r["usable"] == usable
    assert np.array_equal(r["centers"], np.clip(np.rint(want / observed * usable), 128, usable - 1 - 128).astype(np.int32))
    with pytest.raises(ValueError):
        D.clip_rule(cfg, "train", n_frames, cols)                  # random sampling needs its variate


def test_estimation_datasets_are_refused():
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Estimation.yaml"))
    with pytest.raises(NotImplementedError, match="forecast"):
        D.clip_rule(cfg, "test", 150, 1001)


def _stub_loader(label_end, seed=3, mode="train"):
    """A ClipLoader over a store that holds tables only: 4 resident clips of 150 frames / 1001 columns, clip i starting at label
    row 150 i of one label table of label_end[i] rows."""
    cfg = load_yaml(EGO)
    n = len(label_end)
    st = types.SimpleNamespace(
        cfg=cfg, split=mode, nbins=256, n_frames=np.full(n, 150), cols=np.full(n, 1001), slot=np.arange(n), resident=np.arange(n),
        label_first=150 * np.arange(n), label_end=np.asarray(label_end), clips=[("v", f"v_t{5 * i}_t{5 * i + 5}", 5 * i, 5 * i + 5)
                                                                               for i in range(n)],
        clips_host=np.tile(np.array([[0, 86, 36, 48]]), (n, 1)), specs_host=np.tile(np.array([[0, 1001, 573]]), (n, 1)),
        budget_bytes=lambda: None)
    loader = D.ClipLoader(st, batch=2, seed=seed)
    loader.rng = np.random.default_rng((seed, 0))
    return loader


def test_replacement_when_label_rows_run_out():
    # clip 3's table ends at row 3 * 150 + 100: its targets (up to row 149 of the clip at the latest) run out for every u
    ends = [600, 600, 600, 3 * 150 + 64]
    a = _stub_loader(ends)
    ids, tab = a.table([3, 0])
    assert ids[0] != 3 and ids[1] == 0 and a.replaced >= 1
    T = 8
    rows = tab[:, 7:7 + T]
    assert (rows[:, -1] < 600).all() and (rows[0] >= 150 * ids[0]).all() and (rows[0] < 150 * (ids[0] + 1)).all()
    b = _stub_loader(ends)
    ids2, tab2 = b.table([3, 0])
    assert np.array_equal(ids, ids2) and np.array_equal(tab, tab2) and a.replaced == b.replaced      # the same seed repeats
    c = _stub_loader([600] * 4)
    ids3, _ = c.table([3, 0])
    assert ids3.tolist() == [3, 0] and c.replaced == 0
    # the test split takes its clips as they are: a table that runs out is an error that names the clip
    d = _stub_loader(ends, mode="test")
    with pytest.raises(ValueError, match="v_t15_t20"):
        d.table([3])


def test_plan_epoch_train():
    n, batch, world = 23, 2, 3
    per_rank = [D.plan_epoch(n, batch, world, r, 7, 0, True) for r in range(world)]
    assert all(len(g) == 1 for g in per_rank)
    steps = {len(g[0]) for g in per_rank}
    assert len(steps) == 1                                                     # every rank runs the same number of steps
    seen = np.concatenate([np.concatenate(g[0]) for g in per_rank])
    assert len(seen) == len(set(seen.tolist())) and n - len(seen) < batch * world and set(seen.tolist()) <= set(range(n))
    assert all(len(ids) == batch for g in per_rank for ids in g[0])
    again = D.plan_epoch(n, batch, world, 1, 7, 0, True)
    assert all(np.array_equal(x, y) for x, y in zip(again[0], per_rank[1][0]))
    other = D.plan_epoch(n, batch, world, 1, 7, 1, True)
    assert not all(np.array_equal(x, y) for x, y in zip(other[0], per_rank[1][0]))


def test_plan_epoch_eval_keeps_order_and_short_batch():
    groups = D.plan_epoch(7, 3, 1, 0, 7, 5, False)
    assert [ids.tolist() for ids in groups[0]] == [[0, 1, 2], [3, 4, 5], [6]]
    two = [D.plan_epoch(7, 2, 2, r, 7, 0, False) for r in range(2)]
    seen = sorted(np.concatenate([np.concatenate(g[0]) for g in two]).tolist())
    assert seen == list(range(7))


def test_plan_epoch_groups_respect_the_sizes():
    sizes = np.array([10, 30, 20, 10, 40, 10, 20, 30, 10, 10, 20])
    one = D.plan_epoch(len(sizes), 2, 1, 0, 7, 0, True)
    groups = D.plan_epoch(len(sizes), 2, 1, 0, 7, 0, True, group_sizes=(sizes, 70))
    assert len(groups) > 1
    flat = [ids for g in groups for ids in g]
    assert len(flat) == len(one[0]) and all(np.array_equal(x, y) for x, y in zip(flat, one[0]))    # still the same permutation
    for g in groups:
        assert int(sizes[np.unique(np.concatenate(g))].sum()) <= 70
    with pytest.raises(ValueError):
        D.plan_epoch(len(sizes), 2, 1, 0, 7, 0, True, group_sizes=(sizes, 15))


def test_label_columns(tmp_path):
    p = tmp_path / "v_frame_label.csv"
    p.write_text("frame,time,x,y,type\n0,0.00,0.25,0.5,1\n1,0.05,0.75,0.125,0\n2,0.10,0.5,0.5,1\n")
    ego = D.read_labels(str(p), D.dataset_rule("ego4d_av_gaze_forecast")[2])
    aria = D.read_labels(str(p), D.dataset_rule("aria_av_gaze_forecast")[2])
    assert ego.shape == (3, 4) and ego[1].tolist() == [0.05, 0.75, 0.125, 0.0]           # [1:]
    assert aria.shape == (3, 3) and aria.tolist() == [[0.25, 0.5, 1.0], [0.75, 0.125, 0.0], [0.5, 0.5, 1.0]]      # [2:]


def test_split_list_and_missing_files(tmp_path):
    (tmp_path / "train.csv").write_text("a/b/vid/vid_t10_t15.mp4\nvid/vid_t0_t5.avi\n")
    assert D.read_split(str(tmp_path), "train") == [("vid", "vid_t10_t15", 10, 15), ("vid", "vid_t0_t5", 0, 5)]
    with pytest.raises(FileNotFoundError, match="test.csv"):
        D.read_split(str(tmp_path), "val")


def test_config_needs_a_data_root():
    cfg = load_yaml(EGO, ["CSTS_AMD.SYNTHETIC_DATA", False])
    with pytest.raises(ValueError, match="DATA_ROOT"):
        assert_and_infer_cfg(cfg)
    assert_and_infer_cfg(load_yaml(EGO, ["NUM_GPUS", 1, "CSTS_AMD.SYNTHETIC_DATA", False, "CSTS_AMD.DATA_ROOT", "/somewhere"]))
    assert_and_infer_cfg(load_yaml(EGO))


def test_both_libraries_export_the_batch_kernels():
    names = ("csts_batch_sample", "csts_batch_params", "csts_audio_gather")
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    for name in names:
        assert name in lib.SYMBOLS and f"int {name}(" in hdr
    for path in lib._PATHS.values():
        handle = ctypes.CDLL(path)
        for name in names:
            assert hasattr(handle, name), f"{path} does not export {name}"
