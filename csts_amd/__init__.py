"""csts_amd: MI355X-native (gfx950) implementation of the CSTS audio-visual gaze-anticipation training path.

Python host code on PyTorch-ROCm over a C-ABI kernel library (csts_amd/libcsts_hip.so, include/csts_hip.h).
Importing the package is cheap and GPU-free; the kernel library is loaded on first use and its absence is a
hard error (there is no CPU fallback)."""
from .registry import MODEL_REGISTRY  # noqa: F401
from .config import get_cfg, load_yaml, assert_and_infer_cfg  # noqa: F401
from .build import build_model  # noqa: F401
from .infer import GazePredictor, GraphedEvalStep, plan_video, points_to_source, marker_centers  # noqa: F401
from .infer import overlay_group_table  # noqa: F401
from .infer import fill_track, fill_plan, default_max_gap, fill_attention_track, default_attention_gap  # noqa: F401
from .stream import GazeStream, plan_stream, stream_window, stream_schedule, track_from_windows  # noqa: F401
from .stream import stream_live_schedule, live_ring_slots, GazeStreamGroup, group_schedule  # noqa: F401
from .stream import GazeLiveGroup, group_live_schedule  # noqa: F401
from .stream import default_attention_age, attention_ring_slots, live_attention_schedule, attention_track_from_windows  # noqa: F401
from .ops import gaze_overlay, gaze_overlay_yuv, jet_table, audio_pixel_attn, attention_track, attention_rescale  # noqa: F401
from .ops import group_gaze_overlay, group_points_source  # noqa: F401

__all__ = ["MODEL_REGISTRY", "build_model", "get_cfg", "load_yaml", "assert_and_infer_cfg", "GazePredictor", "GraphedEvalStep",
           "plan_video", "fill_track", "fill_plan", "default_max_gap", "points_to_source", "marker_centers", "gaze_overlay",
           "gaze_overlay_yuv",
           "jet_table", "audio_pixel_attn", "attention_track", "attention_rescale", "fill_attention_track",
           "default_attention_gap", "GazeStream", "plan_stream", "stream_window", "stream_schedule", "track_from_windows",
           "stream_live_schedule", "live_ring_slots", "GazeStreamGroup", "group_schedule",
           "GazeLiveGroup", "group_live_schedule", "overlay_group_table", "group_gaze_overlay", "group_points_source",
           "default_attention_age", "attention_ring_slots", "live_attention_schedule", "attention_track_from_windows"]
