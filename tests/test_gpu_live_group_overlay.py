"""GazeLiveGroup's per-size work in one launch each: a round computes the points_source of all slots with ONE
ops.group_points_source and draws all their overlays with ONE ops.group_gaze_overlay, and the bytes are those the per-slot path
gave: each slot's overlay is predictor.render_track of its frames with its rows, its points_source is infer.points_to_source, bit
for bit.  The recordings and ticks of tests/test_gpu_live_group.py, restated: 104 frames of 64 x 80, 104 of 48 x 64, 95 of
64 x 80, 800 samples a frame, ticks of 13 frames, stride 9, bf16, random weights."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import GazePredictor, inputs, ops, points_to_source  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
STRIDE, PER, S = 9, 800, 256
SHAPES = [(104, 64, 80), (104, 48, 64), (95, 64, 80)]
COUNTED = ("group_points_source", "group_gaze_overlay", "gaze_overlay", "gaze_overlay_yuv")


def bits64(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and \
        torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.fixture(scope="module")
def env():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    recs, yuv = [], []
    for i, (n, H, W) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(40 + i)
        recs.append({"frames": torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(DEV),
                     "wav": (0.1 * torch.randn(n * PER, generator=g)).to(DEV)})
        yuv.append(dict(recs[i], frames=torch.randint(0, 256, (n, H * 3 // 2, W), generator=g, dtype=torch.uint8).to(DEV)))
    return {"predictor": predictor, "rgb24": recs, "nv12": yuv}


def replay(group, recs, k=13, ticks=None):
    """Every slot pushes k frames and their audio per tick until its recording ends -> {slot: its live dicts joined}."""
    lives = {}
    starts = list(range(0, max(n for n, _, _ in SHAPES), k))
    for a in starts[:ticks]:
        pieces = {i: (recs[i]["frames"][a:a + k], recs[i]["wav"][a * PER:(a + k) * PER]) for i, (n, _, _) in enumerate(SHAPES) if a < n}
        _, rows = group.push_live(pieces)
        for i in pieces:
            lives.setdefault(i, []).append(rows[i])
    return {i: {key: torch.cat([r[key] for r in rs], dim=0) for key in rs[0]} for i, rs in lives.items()}


class Counters:
    """Counts the calls of the overlay ops and of predictor.render_track while a monkeypatch holds."""

    def __init__(self, monkeypatch, predictor):
        self.calls = dict.fromkeys(COUNTED + ("render_track",), 0)
        for name in COUNTED:
            monkeypatch.setattr(ops, name, self._counted(name, getattr(ops, name)))
        monkeypatch.setattr(predictor, "render_track", self._counted("render_track", predictor.render_track))

    def _counted(self, name, fn):
        def call(*args, **kwargs):
            self.calls[name] += 1
            return fn(*args, **kwargs)
        return call

    def take(self):
        out = dict(self.calls)
        self.calls = dict.fromkeys(self.calls, 0)
        return out


@pytest.mark.parametrize("pixel_format", ["rgb24", "nv12"])
def test_overlay_and_points_source_are_the_per_slot_ones(env, pixel_format):
    p, recs = env["predictor"], env[pixel_format]
    fmt, out_fmt = {}, {}
    if pixel_format == "nv12":
        fmt = {"pixel_format": "nv12", "matrix": "bt709", "full_range": False}
        out_fmt = {"overlay_format": "nv12"}
    group = p.live_group(3, "linear", stride=STRIDE, overlay=True, alpha=0.5, radius=3, **fmt, **out_fmt)
    lives = replay(group, recs)
    for i, (n, H, W) in enumerate(SHAPES):
        live = lives[i]
        shape = (n, H * 3 // 2, W) if fmt else (n, H, W, 3)
        assert live["overlay"].dtype == torch.uint8 and tuple(live["overlay"].shape) == shape
        want = p.render_track(recs[i]["frames"], live, alpha=0.5, radius=3, out_format=out_fmt.get("overlay_format"), **fmt)
        assert torch.equal(live["overlay"], want), i
        nothing = live["neighbours"][:, 0] < 0
        assert 0 < int(nothing.sum()) < n
        assert torch.equal(live["overlay"][nothing], recs[i]["frames"][nothing])
        assert not torch.equal(live["overlay"][~nothing], recs[i]["frames"][~nothing])
        assert bits64(live["points_source"], points_to_source(live["points"], p._video_params_row(H, W), S)), i
        assert int(live["points_source"].isnan().any(dim=-1).sum()) == int(nothing.sum())


def test_a_round_is_one_points_launch_and_one_overlay_launch(env, monkeypatch):
    p, recs = env["predictor"], env["rgb24"]
    group = p.live_group(3, "hold", stride=STRIDE, overlay=True)
    c = Counters(monkeypatch, p)
    for t in range(11):                                           # ticks 0..9 run no window, tick 10 (frames 80..87) runs three
        a = 8 * t
        windows, live = group.push_live({i: (recs[i]["frames"][a:a + 8], recs[i]["wav"][a * PER:(a + 8) * PER]) for i in range(3)})
        assert sum(len(w) for w in windows.values()) == (3 if t == 10 else 0)
        assert c.take() == {"group_points_source": 1, "group_gaze_overlay": 1, "gaze_overlay": 0, "gaze_overlay_yuv": 0,
                            "render_track": 0}, t
        assert all(tuple(live[i]["overlay"].shape) == (8,) + tuple(recs[i]["frames"].shape[1:]) for i in range(3))
    # 16 frames of two slots: two rounds of max_chunk = 8 frames
    small = p.live_group(2, "hold", stride=STRIDE, overlay=True, max_chunk=8)
    c.take()
    small.push_live({i: (recs[i]["frames"][:16], recs[i]["wav"][:16 * PER]) for i in range(2)})
    assert c.take() == {"group_points_source": 2, "group_gaze_overlay": 2, "gaze_overlay": 0, "gaze_overlay_yuv": 0, "render_track": 0}
    # without overlay the fused points_source is all that runs
    plain = p.live_group(3, "hold", stride=STRIDE)
    _, live = plain.push_live({i: (recs[i]["frames"][:8], recs[i]["wav"][:8 * PER]) for i in range(3)})
    assert c.take() == {"group_points_source": 1, "group_gaze_overlay": 0, "gaze_overlay": 0, "gaze_overlay_yuv": 0, "render_track": 0}
    assert all("overlay" not in live[i] and tuple(live[i]["points_source"].shape) == (8, 2) for i in range(3))
    # a tick without frames launches neither
    windows, live = group.push_live({0: (None, recs[0]["wav"][:0]), 1: (None, None)})
    assert sum(c.take().values()) == 0 and windows == {0: [], 1: []}
    assert tuple(live[0]["overlay"].shape) == (0, 64, 80, 3) and tuple(live[1]["points_source"].shape) == (0, 2)


def test_nv12_in_with_rgb_out_stays_per_slot_and_keeps_its_bytes(env, monkeypatch):
    p, recs = env["predictor"], env["nv12"]
    fmt = {"pixel_format": "nv12", "matrix": "bt709", "full_range": False}
    group = p.live_group(3, "linear", stride=STRIDE, overlay=True, alpha=0.5, radius=3, **fmt)
    c = Counters(monkeypatch, p)
    lives = replay(group, recs, ticks=7)                          # 91 frames: one window has run
    seen = c.take()
    assert seen["render_track"] == 3 * 7 and seen["group_points_source"] == 7 and seen["group_gaze_overlay"] == 0
    assert seen["gaze_overlay"] == 3 * 7 and seen["gaze_overlay_yuv"] == 0
    for i, (n, H, W) in enumerate(SHAPES):
        live = lives[i]
        assert tuple(live["overlay"].shape) == (91, H, W, 3)
        want = p.render_track(recs[i]["frames"][:91], live, alpha=0.5, radius=3, **fmt)
        assert torch.equal(live["overlay"], want), i
        rgb = inputs.yuv_to_rgb(recs[i]["frames"][:91], **fmt)
        assert int((live["neighbours"][:, 0] >= 0).sum()) > 0 and not torch.equal(live["overlay"], rgb)
        assert bits64(live["points_source"], points_to_source(live["points"], p._video_params_row(H, W), S))
