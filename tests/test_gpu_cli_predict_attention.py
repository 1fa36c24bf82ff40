"""tools/predict.py --attention / --attention-dir in a child process: the npz gains exactly the fusion attention arrays, the
directory the per-head pictures and the temporal matrices; without the flags the file list is what it was."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
OPTS = ["NUM_GPUS", "1", "TEST.BATCH_SIZE", "3", "CSTS_AMD.COMPUTE", "fp32"]
PREDICT = os.path.join(ROOT, "tools", "predict.py")
PLAIN = ["heatmaps", "peak", "points", "rescaled"]
B, T, H, W = 1, 8, 64, 80
ATTENTION = {"audio_attention": (8, 4, 8, 8), "audio_attention_mean": (4, 8, 8), "attention_maps": (9, T, 8, 8),
             "attention_range": (9, T, 2), "temporal_attention": (8, 8)}


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _run(tmp_path, name, extra):
    out = str(tmp_path / name)
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--out", out] + extra + OPTS, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1 and recs[0]["_type"] == "predict"
    return np.load(out), recs[0], p.stdout


def test_attention_flag_adds_exactly_the_attention_arrays(tmp_path):
    z, rec, _ = _run(tmp_path, "a.npz", ["--attention", "--batch", "2"])
    assert sorted(z.files) == sorted(PLAIN + list(ATTENTION)) and sorted(rec["shapes"]) == sorted(z.files)
    for k, shape in ATTENTION.items():
        assert z[k].shape == (2,) + shape and z[k].dtype == np.float32 and rec["shapes"][k] == [2] + list(shape), k
    assert np.isfinite(z["attention_maps"]).all() and (z["audio_attention"] > 0).all()
    assert np.allclose(z["audio_attention"].mean(axis=1), z["audio_attention_mean"], rtol=1e-5, atol=0)


def test_without_the_flag_the_file_list_is_unchanged(tmp_path):
    z, rec, _ = _run(tmp_path, "plain.npz", ["--batch", "2"])
    assert sorted(z.files) == PLAIN and sorted(rec["shapes"]) == PLAIN


def test_attention_dir_writes_the_pictures_and_the_temporal_matrices(tmp_path):
    g = torch.Generator().manual_seed(22)
    clip = str(tmp_path / "clip.npz")
    np.savez(clip, frames_u8=torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8).numpy(),
             wav=(0.1 * torch.randn(B, 24000 * 5, generator=g)).numpy(),
             frames_idx=(np.arange(T, dtype=np.float32) + 0.5)[None].repeat(B, 0), frame_length=np.float64(T))
    d = tmp_path / "attn"
    z, _, stdout = _run(tmp_path, "c.npz", ["--clip", clip, "--attention-dir", str(d)])       # implies --attention
    assert sorted(z.files) == sorted(PLAIN + list(ATTENTION))
    names = sorted(os.listdir(d))
    texts = [n for n in names if n.endswith(".txt")]
    assert texts == [f"temporal_attn_{b}.txt" for b in range(B)]
    assert np.allclose(np.loadtxt(d / texts[0]), z["temporal_attention"][0], rtol=1e-6, atol=0)
    pngs = [n for n in names if n.endswith(".png")]
    try:
        from PIL import Image
    except ImportError:
        assert pngs == [] and "PIL is not installed" in stdout
        return
    want = [f"spat_attn_{b}_{t}_head_{k}.png" for b in range(B) for t in range(T) for k in list(range(8)) + ["mean"]]
    assert pngs == sorted(want)
    with Image.open(d / "spat_attn_0_0_head_mean.png") as im:
        assert im.size == (W, H) and im.mode == "RGB"
