"""Recorded clips kept as 4:2:0 pictures (csts_amd.datasets): a toy data set written with pixel_format nv12 and its twin holding
the same pictures converted to frames_u8 (inputs.yuv_to_rgb_host) give equal batches bit for bit; the store keeps exactly half
the frame bytes, so a CSTS_AMD.DATA_RESIDENT_GB budget that cuts the RGB split into groups cuts the 4:2:0 split into fewer; a
split mixing formats is refused by the name of the first clip that differs."""
import os
import shutil
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
SIZES = ((96, 128), (100, 120))       # frames large enough to outweigh the clip's spectrogram (1 MB) in the resident budget
OPTS = ["NUM_GPUS", 1, "DATA.TRAIN_CROP_SIZE", S, "DATA.TEST_CROP_SIZE", S, "DATA.TRAIN_JITTER_SCALES", [32, 40],
        "CSTS_AMD.SYNTHETIC_DATA", False]


def _clip_files(root):
    for d, _, files in os.walk(os.path.join(root, "clips")):
        for f in sorted(files):
            yield os.path.join(d, f)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """(the nv12 data set, its RGB twin)."""
    yuv = str(tmp_path_factory.mktemp("toy_nv12"))
    write_dataset(yuv, clips_per_video=(3, 2), sizes=SIZES, test_clips=5, seed=1, pixel_format="nv12")
    rgb = str(tmp_path_factory.mktemp("twin")) + "/rgb"
    shutil.copytree(yuv, rgb)
    for path in _clip_files(rgb):
        with np.load(path) as z:
            rest = {k: z[k] for k in z.files if k not in ("frames_yuv", "pixel_format")}
            frames = inputs.yuv_to_rgb_host(z["frames_yuv"], str(z["pixel_format"]))
        np.savez(path, frames_u8=frames, **rest)
    return yuv, rgb


def _cfg(root, *more):
    return load_yaml(YAML, OPTS + ["CSTS_AMD.DATA_ROOT", root] + list(more))


@pytest.mark.parametrize("mode", ["train", "test"])
def test_batches_equal_those_of_the_rgb_twin(roots, mode):
    stores = [D.ClipStore(_cfg(r), mode, DEV) for r in roots]
    yuv, rgb = stores
    assert yuv.pixel_format == "nv12" and rgb.pixel_format == "rgb24" and yuv.format_args()["matrix"] == "bt601"
    assert yuv.hw.tolist() == rgb.hw.tolist() == [list(SIZES[0])] * 3 + [list(SIZES[1])] * 2
    assert all(f.shape == (86, h * 3 // 2, w) for f, (h, w) in zip(yuv.frames_host, yuv.hw.tolist()))
    assert np.array_equal(yuv.frame_bytes * 2, rgb.frame_bytes)                # exactly half
    assert np.array_equal(yuv.clip_bytes - yuv.frame_bytes, rgb.clip_bytes - rgb.frame_bytes)
    key = torch.tensor([0x0BAD_CAFE_1234_5678], dtype=torch.int64, device=DEV)
    got, want = [], []
    for store, sink in ((yuv, got), (rgb, want)):
        loader = D.ClipLoader(store, batch=3, seed=5)
        for ids in ([0, 3, 4], [2, 1]):
            sink.append(loader.batch(np.array(ids), key=key if mode == "train" else None))
    for a, b in zip(got, want):
        assert np.array_equal(a["clip_ids"], b["clip_ids"])
        for k in ("video", "audio", "labels", "labels_hm", "frames_idx", "params"):
            assert torch.equal(a[k], b[k]), k
        assert bool(torch.isfinite(a["video"]).all())


def test_the_budget_holds_more_clips(roots):
    yuv, rgb = (D.ClipStore(_cfg(r), "test", DEV) for r in roots)
    # the two largest RGB clips fit the budget together, three do not
    budget = int(np.sort(rgb.clip_bytes)[-2:].sum() + 64)
    plans = []
    for root, store in zip(roots, (yuv, rgb)):
        s = D.ClipStore(_cfg(root, "CSTS_AMD.DATA_RESIDENT_GB", budget / 2 ** 30), "test", DEV)
        plans.append(D.ClipLoader(s, batch=1).plan(0))
    k_yuv, k_rgb = len(plans[0]), len(plans[1])
    assert (k_yuv, k_rgb) == (2, 3)                                            # 3 + 2 clips against 2 + 2 + 1
    assert sum(len(g) for g in plans[0]) == sum(len(g) for g in plans[1]) == 5


def test_a_split_mixing_formats_is_refused(roots, tmp_path):
    yuv, rgb = roots
    mixed = str(tmp_path / "mixed")
    shutil.copytree(yuv, mixed)
    name = os.path.join("clips", "video01", "video01_t0_t5.npz")
    shutil.copy(os.path.join(rgb, name), os.path.join(mixed, name))
    with pytest.raises(ValueError, match="video01_t0_t5.*uniform"):
        D.ClipStore(_cfg(mixed), "train", DEV)
    # the same layout under another matrix differs too
    other = str(tmp_path / "matrix")
    shutil.copytree(yuv, other)
    path = os.path.join(other, "clips", "video00", "video00_t10_t15.npz")
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    np.savez(path, yuv_matrix=np.array("bt709"), **arrays)
    with pytest.raises(ValueError, match="video00_t10_t15.*uniform"):
        D.ClipStore(_cfg(other), "train", DEV)
    both = str(tmp_path / "both")
    shutil.copytree(yuv, both)
    path = os.path.join(both, "clips", "video00", "video00_t0_t5.npz")
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    np.savez(path, frames_u8=np.zeros((150,) + SIZES[0] + (3,), np.uint8), **arrays)
    with pytest.raises(ValueError, match="both frames_u8 and frames_yuv"):
        D.ClipStore(_cfg(both), "train", DEV)
