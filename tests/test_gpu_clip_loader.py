"""csts_amd.datasets.ClipStore / ClipLoader on a toy data set (2 videos of 36 x 48 and 40 x 44 frames, 5 clips of 150 frames, 5 s
of noise each): a batch equals, bit for bit, the same batch rebuilt per clip from the single-recording ops (spatial_sampling's
rule, clip_sample, audio_windows_at, gaze_heatmaps) using the clip numbers, frame numbers and key the loader returns; an epoch
uploaded in two groups under CSTS_AMD.DATA_RESIDENT_GB yields the batches of the epoch uploaded at once."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import datasets as D, inputs  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402
from make_toy_dataset import write_dataset  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
S = 32
OPTS = ["NUM_GPUS", 1, "DATA.TRAIN_CROP_SIZE", S, "DATA.TEST_CROP_SIZE", S, "DATA.TRAIN_JITTER_SCALES", [32, 40],
        "CSTS_AMD.SYNTHETIC_DATA", False]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("toy"))
    write_dataset(out, clips_per_video=(3, 2), sizes=((36, 48), (40, 44)), test_clips=5, seed=1)
    return out


def _cfg(root, *more):
    return load_yaml(YAML, OPTS + ["CSTS_AMD.DATA_ROOT", root] + list(more))


def _rebuilt(store, loader, batch):
    """The batch from the single-recording ops, clip by clip."""
    cfg, T = store.cfg, loader.T
    ids, idx = batch["clip_ids"], batch["frames_idx"]
    video, audio, labels, hm = [], [], [], []
    for b, i in enumerate(ids.tolist()):
        frames = torch.from_numpy(store.frames_host[i]).to(DEV)                 # (86, H, W, 3)
        spec = torch.from_numpy(store.spec_host[i]).to(DEV)
        rule_idx = idx[b].cpu().numpy().astype(np.int64)
        # label rows and centres follow from the returned frames by the dataset's rule
        n, obs, usable = int(store.n_frames[i]), store.observed, int(store.usable[i])
        if loader.train:
            last = int(rule_idx[-1])
            rows = np.linspace(last + 1, last + n - obs, T).astype(np.int64)
        else:
            rows = np.linspace(obs, n - 1, T).astype(np.int64)
        lab = store.labels_host[store.label_first[i] + rows][None]             # (1, T, L)
        H, W = frames.shape[1:3]
        if loader.train:
            key = int(batch["key"].item())
            u = inputs.spatial_uniforms_host(key, b, 1)                         # clip b of the batch draws u[b]
            par, new = inputs.spatial_rule_host(lab, H, W, S, uniforms=u, **loader.spatial_args())
        else:
            par, new = inputs.spatial_rule_host(lab, H, W, S, **loader.spatial_args())
        par = torch.from_numpy(par).to(DEV)
        video.append(inputs.clip_sample(frames, idx[b:b + 1], par, S, mean=tuple(cfg.DATA.MEAN), std=tuple(cfg.DATA.STD)))
        cen = np.clip(np.rint(rule_idx.astype(np.float64) / obs * usable), 128, usable - 1 - 128).astype(np.int32)
        win = inputs.audio_windows_at(spec[:, :usable].contiguous(), torch.from_numpy(cen[None]).to(DEV), 256)
        o = (256 - S) // 2
        audio.append(win[:, :, :, :S, o:o + S].contiguous())
        new = torch.from_numpy(new).to(DEV)
        labels.append(new)
        hm.append(inputs.gaze_heatmaps(new, H=S // 4, W=S // 4))
    return {"video": torch.cat(video), "audio": torch.cat(audio), "labels": torch.cat(labels), "labels_hm": torch.cat(hm)}


@pytest.mark.parametrize("mode", ["train", "test"])
def test_batch_equals_the_rebuilt_batch(root, mode):
    cfg = _cfg(root)
    store = D.ClipStore(cfg, mode, DEV)
    assert len(store) == 5 and store.hw.tolist() == [[36, 48]] * 3 + [[40, 44]] * 2 and store.labels.dtype == torch.float64
    assert all(f.shape[0] == 86 for f in store.frames_host)                     # the observed part only
    loader = D.ClipLoader(store, batch=3, seed=5)
    torch.manual_seed(9)
    batches = list(loader.epoch(0))
    assert [len(b["clip_ids"]) for b in batches] == ([3] if mode == "train" else [3, 2])     # train drops the short batch
    for batch in batches:
        B = len(batch["clip_ids"])
        assert batch["video"].shape == (B, 3, 8, S, S) and batch["audio"].shape == (B, 1, 8, S, S)
        assert batch["labels_hm"].shape == (B, 8, S // 4, S // 4) and batch["labels"].dtype == torch.float64
        assert (batch["key"] is None) == (mode != "train")
        want = _rebuilt(store, loader, batch)
        for k in ("video", "audio", "labels", "labels_hm"):
            assert torch.equal(batch[k], want[k]), k
        assert bool(torch.isfinite(batch["video"]).all())


def test_two_groups_yield_the_batches_of_one(root):
    store = D.ClipStore(_cfg(root), "train", DEV)
    one = D.ClipLoader(store, batch=2, seed=5)
    torch.manual_seed(9)
    a = list(one.epoch(3))
    assert store.uploads == 1 and len(a) == 2
    # two clips and their spectrograms fit the budget, four do not
    gb = float(np.sort(store.clip_bytes)[-2:].sum() + 64) / 2 ** 30
    store2 = D.ClipStore(_cfg(root, "CSTS_AMD.DATA_RESIDENT_GB", gb), "train", DEV)
    two = D.ClipLoader(store2, batch=2, seed=5)
    logged = []
    torch.manual_seed(9)
    b = list(two.epoch(3, log=logged.append))
    assert store2.uploads == 2 and len(logged) == 1 and logged[0]["groups"] == 2
    assert len(b) == len(a)
    for x, y in zip(a, b):
        assert np.array_equal(x["clip_ids"], y["clip_ids"]) and torch.equal(x["key"], y["key"])
        for k in ("video", "audio", "labels", "labels_hm", "frames_idx"):
            assert torch.equal(x[k], y[k]), k


def test_missing_clip_and_budget_errors_name_their_cause(root, tmp_path):
    import shutil
    bad = str(tmp_path / "bad")
    shutil.copytree(root, bad)
    os.remove(os.path.join(bad, "clips", "video01", "video01_t5_t10.npz"))
    with pytest.raises(FileNotFoundError, match="video01_t5_t10"):
        D.ClipStore(_cfg(bad), "train", DEV)
    store = D.ClipStore(_cfg(root, "CSTS_AMD.DATA_RESIDENT_GB", 1e-6), "train", DEV)
    with pytest.raises(ValueError, match="DATA_RESIDENT_GB"):
        list(D.ClipLoader(store, batch=2).epoch(0))
    with pytest.raises(NotImplementedError, match="estimation"):
        D.ClipStore(_cfg(root, "TRAIN.DATASET", "ego4d_av_gaze"), "train", DEV)
