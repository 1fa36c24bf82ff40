"""Inference: trained weights in, gaze predictions out.

``GazePredictor`` is the public interface: it builds the model, loads a checkpoint by the reference's name-and-shape rule
(csts_amd.checkpoint) and turns uint8 frames + a waveform into a gaze point, its probability and the heat map of every frame,
all on the device.  What the reference's test driver does per batch (tools/test_avgaze_net.py:50-70: eval forward,
frame_softmax at temperature 2, per-frame min-max rescale) runs here as the model forward followed by ONE fused head kernel
(csts_gaze_decode), and ``GraphedEvalStep`` captures the two into one HIP graph: the forward is launch-bound from Python just
as the training step is, so replaying it is the eval counterpart of train.GraphedTrainStep."""
from __future__ import annotations

import torch

from . import checkpoint as ck
from . import lib as L
from . import ops

TEMPERATURE = 2.0          # frame_softmax temperature of the train / val / test drivers of the reference
AUDIO_WIDTH = 256          # spectrogram columns per audio window (ego4d_avgaze_forecast.py:218-219)


def window_rule(cfg, fps=None, stride=None, segment=None):
    """The part of plan_video that does not need the recording's length (plan_stream shares it): the table of the dataset
    cfg.TEST.DATASET names -> {"segment", "observed", "stride", "clip_size", "inputs" and "targets" int64 (T,) local to a window's
    origin}, as plan_video's docstring states them."""
    import math
    import numpy as np
    from .inputs import temporal_indices
    T, rate, target_fps = int(cfg.DATA.NUM_FRAMES), int(cfg.DATA.SAMPLING_RATE), cfg.DATA.TARGET_FPS
    fps = target_fps if fps is None else fps
    views = int(cfg.TEST.NUM_ENSEMBLE_VIEWS)
    name = str(cfg.TEST.DATASET).lower()
    clip_size = ((rate + 1) * (T - 1) + 1) / target_fps * fps
    if "forecast" in name:
        seg0, obs0, first0 = (100, 60, 60 + rate) if "aria" in name else (150, 86, 86)
        seg = seg0 if segment is None else int(segment)
        if seg < 1:
            raise ValueError(f"segment must be positive, got {segment}")
        observed = obs0 * seg // seg0
        if observed < 1 or observed >= seg:
            raise ValueError(f"a segment of {seg} frames leaves no observed / predicted part ({observed} observed)")
        targets = np.linspace(first0, seg0 - 1, T).astype(np.int64) * seg // seg0
        _, _, inputs_local = temporal_indices(observed, T, rate, 1, views, target_fps=target_fps, fps=fps)
        default_stride = seg - observed
    else:
        seg = int(round(5 * fps)) if segment is None else int(segment)
        if seg < 1:
            raise ValueError(f"segment must be positive, got {segment}")
        observed = seg
        _, _, inputs_local = temporal_indices(seg, T, rate, 0, views, target_fps=target_fps, fps=fps)
        targets = inputs_local.copy()
        default_stride = int(math.ceil(clip_size))
    stride = default_stride if stride is None else int(stride)
    if stride < 1:
        raise ValueError(f"stride must be positive, got {stride}")
    return {"segment": seg, "observed": observed, "stride": stride, "clip_size": clip_size,
            "inputs": inputs_local.astype(np.int64), "targets": targets.astype(np.int64)}


def plan_video(cfg, n_frames, fps=None, stride=None, segment=None, cols=None):
    """The windows predict_video cuts a recording of n_frames frames into, on the host (numpy arrays).

    A window is one clip of the dataset cfg.TEST.DATASET names: `segment` frames from its origin o_w = w * stride, of which
    the first `observed` are seen.  Its T input frames follow the reference's temporal rule on the observed part
    (inputs.temporal_indices) and its T predictions target
      forecast, not aria: 150 / 86 frames, inputs clip 1 of TEST.NUM_ENSEMBLE_VIEWS, targets linspace(86, 149, T)
                          (ego4d_avgaze_forecast.py:197,234-235);
      forecast and aria:  100 / 60 frames, same inputs, targets linspace(60 + rate, 99, T) (aria_avgaze_forecast.py:192,230-231);
      estimation:         round(5 fps) frames, all observed, inputs clip 0, targets = the input frames (ego4d_avgaze.py:263-267),
    all local to the origin.  Default stride: segment - observed (forecast: the predicted spans tile the video) or
    ceil(clip size) (estimation).  `segment` overrides the table; the forecast rows then scale observed and the targets by
    segment / table segment, floored.  windows = floor((n_frames - observed) / stride) + 1; fewer than `observed` frames is an
    error.  Targets >= n_frames stay in the plan (gaze_track drops them).  fps defaults to DATA.TARGET_FPS.

    cols (optional): the columns of ONE spectrogram of the whole waveform.  The plan then holds the audio window centres by the
    rule of ego4d_avgaze_forecast.py:215-219 applied to the window's slice [c0, c1) = [floor(o cols / n), floor((o + observed)
    cols / n)): centre = c0 + round(local / observed * (c1 - c0)) clipped to [c0 + 128, c1 - 1 - 128]; a slice narrower than
    257 columns is an error.

    Returns {"windows", "segment", "observed", "stride", "clip_size", "origins" (windows,), "inputs" and "targets" (T,) local,
    "frames_idx" int32 and "target_idx" int64 (windows, T) absolute [, "audio_centers" int32 (windows, T)]}."""
    import numpy as np
    n_frames = int(n_frames)
    rule = window_rule(cfg, fps=fps, stride=stride, segment=segment)
    seg, observed, stride, clip_size = rule["segment"], rule["observed"], rule["stride"], rule["clip_size"]
    inputs_local, targets = rule["inputs"], rule["targets"]
    if n_frames < observed:
        raise ValueError(f"the video has {n_frames} frames, one window observes {observed}")
    windows = (n_frames - observed) // stride + 1
    origins = np.arange(windows, dtype=np.int64) * stride
    plan = {"windows": windows, "segment": seg, "observed": observed, "stride": stride, "clip_size": clip_size,
            "origins": origins, "inputs": inputs_local.astype(np.int64), "targets": targets.astype(np.int64),
            "frames_idx": (origins[:, None] + inputs_local[None, :]).astype(np.int32),
            "target_idx": (origins[:, None] + targets[None, :]).astype(np.int64)}
    if cols is not None:
        cols = int(cols)
        c0 = origins * cols // n_frames
        c1 = (origins + observed) * cols // n_frames
        if int((c1 - c0).min()) < AUDIO_WIDTH + 1:
            raise ValueError(f"the spectrogram slice of a window has {int((c1 - c0).min())} columns ({cols} for {n_frames} frames), "
                             f"an audio window needs {AUDIO_WIDTH + 1}")
        centers = c0[:, None] + np.rint(inputs_local[None, :].astype(np.float64) / observed * (c1 - c0)[:, None]).astype(np.int64)
        half = AUDIO_WIDTH // 2
        plan["audio_centers"] = np.clip(centers, (c0 + half)[:, None], (c1 - 1 - half)[:, None]).astype(np.int32)
    return plan


def default_max_gap(plan):
    """The widest step between two consecutive predictions of one window of `plan` (plan_video): max(diff(plan["targets"])) =
    SAMPLING_RATE + 1 for the shipped YAMLs (9 for Ego4D, 5 for Aria).  As the max_gap of fill_track it fills the gaps inside a
    window and the one-frame seam between default-stride windows, and leaves a stretch nobody forecasts empty."""
    import numpy as np
    targets = np.asarray(plan["targets"], dtype=np.int64)
    if targets.size < 2:
        return 1
    return max(1, int(np.diff(targets).max()))


def fill_plan(count, max_gap):
    """The rule of csts_gaze_track_fill (include/csts_hip.h) on the host: count (N,) = windows per frame -> int64 (N, 2)
    neighbours.  A predicted frame n (count > 0) has (n, n).  Any other frame has a = the largest predicted frame below it and
    b = the smallest above it; both exist and b - a <= max_gap: (a, b), the frame is filled; otherwise (-1, -1).  Nothing
    before the first or after the last predicted frame is filled."""
    import numpy as np
    count = np.asarray(count).reshape(-1)
    max_gap = int(max_gap)
    if max_gap < 1:
        raise ValueError(f"max_gap must be positive, got {max_gap}")
    N = count.shape[0]
    idx = np.arange(N, dtype=np.int64)
    pred = count > 0
    a = np.maximum.accumulate(np.where(pred, idx, -1))                             # the last predicted frame <= n
    b = np.minimum.accumulate(np.where(pred, idx, N)[::-1])[::-1]                  # the first predicted frame >= n, N: none
    ok = pred | ((a >= 0) & (b < N) & (b - a <= max_gap))
    return np.where(ok[:, None], np.stack([a, b], axis=-1), -1).astype(np.int64)


def fill_track(track, mode="linear", max_gap=None, plan=None):
    """The sparse track of predict_video with the frames between neighbouring predictions filled (ops.gaze_track_fill,
    csts_gaze_track_fill).  track: a dict with "heatmaps" fp32 (N, h, w) and "count" int32 (N,) on the device -- what
    predict_video returned, or the arrays of its .npz moved to the device.  mode "hold" repeats the earlier map (what the
    reference's visualisation does), "linear" blends the two neighbours by time.  max_gap: the widest distance b - a between
    two predictions that is still filled; None takes default_max_gap(plan) and needs plan= (the plan_video result of the
    recording).  Returns a NEW dict: "heatmaps", "rescaled", "points" and "peak" filled (predicted frames keep their bits),
    "neighbours" int32 (N, 2), "filled" bool (N,) = count == 0 and a neighbour exists, "max_gap" = the gap that was applied
    (a host int); "count" and every other entry as they
    were, except "points_source" and "overlay", which describe the sparse track and are left out.  The input is not modified."""
    if "heatmaps" not in track or "count" not in track:
        raise ValueError("fill_track needs the track's \"heatmaps\" and \"count\": call predict_video with return_heatmaps=True")
    if max_gap is None:
        if plan is None:
            raise ValueError("fill_track needs max_gap, or plan= (the plan_video result) to take default_max_gap from")
        max_gap = default_max_gap(plan)
    out = {k: v for k, v in track.items() if k not in ("points_source", "overlay")}
    out.update(ops.gaze_track_fill(track["heatmaps"], track["count"], mode=mode, max_gap=int(max_gap)))
    out["filled"] = (track["count"] == 0) & (out["neighbours"][:, 0] >= 0)
    out["max_gap"] = int(max_gap)
    return out


def default_attention_gap(plan):
    """The widest step between two consecutive INPUT frames of one window of `plan` (plan_video): max(diff(plan["inputs"])), at
    least 1 -- 9 on the Ego4D forecast plan, 5 on the Aria one.  The attention track lands on the input frames (the frames the
    audio was heard with), not on the predicted ones, so its fill has its own default gap: it fills inside a window's observed
    span and leaves the stretch between two windows' observed spans empty."""
    import numpy as np
    inputs = np.asarray(plan["inputs"], dtype=np.int64)
    if inputs.size < 2:
        return 1
    return max(1, int(np.diff(inputs).max()))


ATTENTION_TRACK_KEYS = ("attention_maps", "attention_range", "attention_mixed", "attention_count")


def attention_grid(cfg, crop_size=None):
    """(heads, T', h, w) of the spatial fusion block, whose attention predict(attention=True) shows, from the configuration alone:
    the encoder's last head count (MVIT.NUM_HEADS through MVIT.HEAD_MUL) and the patch grid of a NUM_FRAMES x S x S clip divided
    by every MVIT.POOL_Q_STRIDE; S = crop_size, default DATA.TEST_CROP_SIZE.  The shipped YAMLs at S = 256: (8, 4, 8, 8).  A
    stream sizes its attention ring by it before any window has run."""
    from .model import round_width
    head_mul = {int(i): m for i, m in cfg.MVIT.HEAD_MUL}
    heads = int(cfg.MVIT.NUM_HEADS)
    for i in range(int(cfg.MVIT.DEPTH)):
        heads = round_width(heads, head_mul.get(i, 1.0))
    S = int(cfg.DATA.TEST_CROP_SIZE if crop_size is None else crop_size)
    grid = [n // int(s) for n, s in zip((int(cfg.DATA.NUM_FRAMES), S, S), cfg.MVIT.PATCH_STRIDE)]
    for row in cfg.MVIT.POOL_Q_STRIDE:
        grid = [n // int(s) for n, s in zip(grid, row[1:])]
    return (int(heads),) + tuple(int(n) for n in grid)


def fill_attention_track(track, mode="linear", max_gap=None, plan=None, crop_size=None):
    """The attention track of predict_video(attention_track=True) with the frames between neighbouring hit frames filled, as
    fill_track fills the gaze track.  track: a dict with "attention_mixed" fp32 (N, heads + 1, h, w) and "attention_count" int32
    (N,) on the device.  The fill runs on the MIXED maps -- ops.gaze_track_fill on the frame's heads + 1 maps viewed as one
    (heads + 1) h x w map, so hold / linear and the neighbour rule are the gaze track's, bit for bit -- and ops.attention_rescale
    then gives every hit or filled frame its own extrema: a blend is rescaled by the range of the blend, a hit frame keeps its
    bits.  max_gap: None takes default_attention_gap(plan) and needs plan=.  crop_size: the S of the lattice; None takes
    track["attention_crop_size"] (predict_video stores it).  Returns a NEW dict: "attention_mixed", "attention_maps" and
    "attention_range" filled, "attention_neighbours" int32 (N, 2), "attention_filled" bool (N,), "attention_max_gap" (a host
    int); every other entry as it was.  The fill kernel holds a frame in registers: (heads + 1) h w <= CSTS_GAZE_DECODE_MAX_HW."""
    if "attention_mixed" not in track or "attention_count" not in track:
        raise ValueError("fill_attention_track needs the track's \"attention_mixed\" and \"attention_count\": call predict_video "
                         "with attention_track=True")
    if max_gap is None:
        if plan is None:
            raise ValueError("fill_attention_track needs max_gap, or plan= (the plan_video result) to take default_attention_gap from")
        max_gap = default_attention_gap(plan)
    if crop_size is None:
        if "attention_crop_size" not in track:
            raise ValueError("fill_attention_track needs crop_size= (DATA.TEST_CROP_SIZE) or the track's \"attention_crop_size\"")
        crop_size = track["attention_crop_size"]
    mixed, count = track["attention_mixed"], track["attention_count"]
    if mixed.dim() != 4:
        raise ValueError(f"attention_mixed must be (N, heads + 1, h, w), got {tuple(mixed.shape)}")
    N, G, h, w = mixed.shape
    if G * h * w > L.GAZE_DECODE_MAX_HW:
        raise ValueError(f"the fill holds a frame's {G} maps of {h} x {w} in registers: (heads + 1) * h * w = {G * h * w} exceeds "
                         f"CSTS_GAZE_DECODE_MAX_HW ({L.GAZE_DECODE_MAX_HW})")
    out = dict(track)
    filled = ops.gaze_track_fill(mixed.contiguous().view(N, G * h, w), count, mode=mode, max_gap=int(max_gap),
                                 want=("heatmaps", "neighbours"))
    out["attention_mixed"] = filled["heatmaps"].view(N, G, h, w)
    out["attention_neighbours"] = filled["neighbours"]
    out["attention_filled"] = (count == 0) & (filled["neighbours"][:, 0] >= 0)
    rescaled = ops.attention_rescale(out["attention_mixed"], int(crop_size), valid=(count > 0) | out["attention_filled"])
    out["attention_maps"], out["attention_range"] = rescaled["maps"], rescaled["range"]
    out["attention_max_gap"] = int(max_gap)
    out["attention_crop_size"] = int(crop_size)
    return out


def points_to_source(points, params_row, crop_size):
    """Gaze points (N, 2) = (x, y) normalised on the S x S crop -> the same points normalised on the SOURCE frame the crop was cut
    from: x_src = (x S + x0) / new w, y_src = (y S + y0) / new h, the inverse of the label rule of the spatial sampling.
    params_row: (new h, new w, y0, x0, flip) on the host.  float64 on the device of `points`; NaN stays NaN."""
    nh, nw, y0, x0 = (int(v) for v in list(params_row)[:4])
    S = float(int(crop_size))
    p = points.to(torch.float64)
    if p.dim() != 2 or p.shape[1] != 2:
        raise ValueError(f"points must be (N, 2), got {tuple(points.shape)}")
    # the divisors are tensors: torch divides a device tensor by a host scalar as a multiplication by its reciprocal, one ulp off
    # the quotient the formula states; tensor / tensor is the IEEE division on either device
    x, y = p[:, 0], p[:, 1]
    return torch.stack([(x * S + float(x0)) / torch.full_like(x, float(nw)), (y * S + float(y0)) / torch.full_like(y, float(nh))],
                       dim=-1)


def marker_centers(points_source, H, W):
    """Source-normalised points (N, 2) -> int32 (N, 2) marker centres (X, Y) = floor(p * (W, H)) in source pixels, (-1, -1) where
    the point is NaN (ops.gaze_overlay leaves such a frame untouched)."""
    p = points_source.to(torch.float64)
    if p.dim() != 2 or p.shape[1] != 2:
        raise ValueError(f"points must be (N, 2), got {tuple(points_source.shape)}")
    c = torch.floor(p * torch.tensor([float(W), float(H)], dtype=torch.float64, device=p.device))
    bad = torch.isnan(p).any(dim=-1, keepdim=True)
    return torch.where(bad, torch.full_like(c, -1.0), c).to(torch.int32)


OVERLAY_BAND_ROWS = 32                                        # frame rows per workgroup of the overlay kernels (OV_ROWS)


def overlay_group_table(sizes, vector=None):
    """The host rule of a grouped overlay launch (ops.group_gaze_overlay, ops.group_points_source; include/csts_hip.h, "gaze
    overlay of a group"): sizes is a list of (K, H, W), one per job, vector the per-job flags of the 4-pixel path (None: a job is
    on it when W % 4 == 0; a flag set on a job whose W % 4 != 0 is a ValueError) -> {"first_row": int64 (J,), the index of a job's
    first row in the concatenated rescaled / centers = the sum of the K before it; "first_workgroup": int64 (J,), the sum of
    K * bands of the jobs before it; "bands": int64 (J,) = ceil(H / 32); "vector": int64 (J,) 0 / 1; "rows": the sum of K;
    "grid": the sum of K * bands}.  Workgroup g belongs to the last job j with first_workgroup[j] <= g, which the kernel finds
    by binary search; inside it, frame (g - first_workgroup[j]) // bands[j] and band (g - first_workgroup[j]) % bands[j].  A job
    with K < 1 or a non-positive size is a ValueError naming the job.  Pure numpy: no GPU."""
    import numpy as np
    sizes = [tuple(int(v) for v in s) for s in sizes]
    J = len(sizes)
    flags = [None] * J if vector is None else list(vector)
    if len(flags) != J:
        raise ValueError(f"vector must hold one flag per job ({J}), got {len(flags)}")
    first_row, first_wg, bands, vec = (np.zeros(J, dtype=np.int64) for _ in range(4))
    rows = grid = 0
    for j, size in enumerate(sizes):
        if len(size) != 3 or min(size) < 1:
            raise ValueError(f"job {j}: (K, H, W) must be three positive integers, got {size}")
        K, H, W = size
        v = W % 4 == 0 if flags[j] is None else bool(flags[j])
        if v and W % 4:
            raise ValueError(f"job {j}: the vector path takes 4 pixels a lane and needs W % 4 == 0, got W {W}")
        first_row[j], first_wg[j], bands[j], vec[j] = rows, grid, -(-H // OVERLAY_BAND_ROWS), int(v)
        rows += K
        grid += K * int(bands[j])
    return {"first_row": first_row, "first_workgroup": first_wg, "bands": bands, "vector": vec, "rows": rows, "grid": grid}


def _core(model):
    return model.module if hasattr(model, "module") else model


# result name of predict(attention=True) -> entry of the model's fusion dict (CSTS.forward_head, return_fusion_maps)
ATTENTION_OUTPUTS = {"audio_attention": "column", "audio_attention_mean": "column_mean", "attention_maps": "maps",
                     "attention_range": "range", "temporal_attention": "temporal"}


def eval_forward(model, video, audio, attention=False):
    """model([video], audio) -> gaze_decode, with the kernels the graph replays.  The caller holds eval mode and no_grad.
    Returns {"logits", "preds", "rescaled"}: (B, 1, T, H/4, W/4); "points": (B, T, 2); "peak": (B, T).  attention=True runs the
    forward with return_fusion_maps and adds the entries of ATTENTION_OUTPUTS; the logits are the same bits either way."""
    if attention:
        logits, fusion = model([video], audio, return_fusion_maps=True)
    else:
        logits = model([video], audio)
    out = ops.gaze_decode(logits, TEMPERATURE)
    out["logits"] = logits
    if attention:
        out.update({k: fusion[v] for k, v in ATTENTION_OUTPUTS.items()})
    return out


class GraphedEvalStep:
    """The forward-only step -- eval-mode model([video], audio), then gaze_decode -- captured ONCE into a HIP graph and replayed.
    The capture runs the model's own forward, so the second-stream trunks of CSTS_AMD.TWO_STREAMS are part of the graph as
    they are in the training capture.  Inputs are copied into static buffers; run() returns the graph's static outputs, which
    the next run() overwrites.  The model's parameters are not touched and its training flag is put back.  attention=True
    captures the forward that also yields the fusion attention maps (eval_forward)."""

    def __init__(self, cfg, model, example_batch, warmup: int = 2, attention: bool = False):
        self.cfg, self.model = cfg, _core(model)      # forward only: nothing for a data-parallel wrapper to reduce
        self.attention = bool(attention)
        for k in ("video", "audio"):
            if not example_batch[k].is_cuda:
                raise L.CstsError("GraphedEvalStep runs on MI355X only: the batch must hold GPU tensors")
        self.static = {k: example_batch[k].detach().clone() for k in ("video", "audio")}
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(max(1, warmup)):      # lazy tables, weight shadows and the allocator see the real thing
                        self._step()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                ops.refill_capture_pools()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                    self.out = self._step()
                torch.cuda.synchronize()
        finally:
            self.model.train(was_training)

    def _step(self):
        return eval_forward(self.model, self.static["video"], self.static["audio"], attention=self.attention)

    def run(self, video=None, audio=None):
        """Copy the inputs into the static buffers (None: keep what they hold) and replay.  Returns the static outputs
        {"logits", "preds", "rescaled", "points", "peak"} (and the ATTENTION_OUTPUTS of a step captured with attention)."""
        for k, v in (("video", video), ("audio", audio)):
            if v is not None and v is not self.static[k]:
                if v.shape != self.static[k].shape:
                    raise ValueError(f"{k} is {tuple(v.shape)}, this step was captured for {tuple(self.static[k].shape)}")
                self.static[k].copy_(v, non_blocking=True)
        if hasattr(self.model, "_refresh_w16"):
            was_training = self.model.training
            self.model.eval()
            try:
                with torch.no_grad():
                    self.model._refresh_w16()        # only acts after an out-of-band weight change (load_state_dict)
            finally:
                self.model.train(was_training)
        self.graph.replay()
        return self.out


def _picture_hw(frames, lead, pixel_format, matrix, full_range, window=None):
    """H, W and the format keywords of a picture argument with `lead` leading dimensions: packed RGB uint8 (..., H, W, 3) -> (H,
    W, {}), or with pixel_format "nv12" | "i420" 4:2:0 uint8 (..., H * 3 / 2, W) -> (H, W, the three keywords to pass on).
    window (top, left, H, W): the frames are 4:2:0 surfaces and the pictures their windows (inputs.check_window): H, W are the
    window's and the keywords carry it.  ValueError for an unknown format or matrix, a shape of the other kind, odd H or W, a
    bad window or a window of packed RGB."""
    from . import inputs
    names = "(B, T" if lead == 2 else "(N"
    if inputs.check_pixel_format(pixel_format, matrix, full_range)[0] == 0:
        inputs.check_window(frames.shape, pixel_format, window)
        if frames.dtype != torch.uint8 or frames.dim() != lead + 3 or frames.shape[-1] != 3:
            raise ValueError(f"frames must be uint8 {names}, H, W, 3), got {tuple(frames.shape)} {frames.dtype}")
        return int(frames.shape[-3]), int(frames.shape[-2]), {}
    if frames.dtype != torch.uint8 or frames.dim() != lead + 2:
        raise ValueError(f"{pixel_format} frames must be uint8 {names}, H * 3 / 2, W), got {tuple(frames.shape)} {frames.dtype}")
    H, W = inputs.window_size(frames.shape, pixel_format, window)
    fmt = {"pixel_format": pixel_format, "matrix": matrix, "full_range": bool(full_range)}
    if window is not None:
        fmt["window"] = tuple(int(v) for v in window)
    return H, W, fmt


def _render_out(frames, out, H, W, fmt):
    """The uint8 (..., H, W, 3) tensor a renderer of 4:2:0 frames draws into: a fresh one unless `out` is given, and `out` must not
    share memory with the input (the RGB pictures are converted into it, then drawn over in place)."""
    shape = tuple(frames.shape[:-2]) + (H, W, 3)
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.uint8 or
                            not out.is_contiguous() or not out.is_cuda):
        raise ValueError(f"out must be a contiguous uint8 {shape} GPU tensor")
    if out is not None:
        a, b = frames.data_ptr(), out.data_ptr()
        if a < b + out.numel() and b < a + frames.numel() * frames.element_size():
            raise ValueError(f"out must not share memory with {fmt['pixel_format']} frames: the overlay is RGB, (N, H, W, 3)")
    return torch.empty(shape, dtype=torch.uint8, device=frames.device) if out is None else out


OVERLAY_FORMATS = (None, "rgb24", "nv12", "i420")


def _overlay_yuv(out_format, fmt, what="out_format"):
    """Whether a renderer draws in 4:2:0 (ops.gaze_overlay_yuv): False for None / "rgb24", True for "nv12" / "i420" on frames of
    that very layout (fmt: the format keywords of _picture_hw, {} for packed RGB).  ValueError for anything else."""
    if out_format is None or out_format == "rgb24":
        return False
    if out_format not in OVERLAY_FORMATS:
        raise ValueError(f"{what} must be None, 'rgb24', 'nv12' or 'i420', got {out_format!r}")
    if not fmt:
        raise ValueError(f"{what}={out_format!r} needs frames in that layout (pixel_format={out_format!r}), these are packed RGB: "
                         "RGB in with 4:2:0 out is inputs.rgb_to_yuv of the RGB overlay")
    if fmt["pixel_format"] != out_format:
        raise ValueError(f"{what}={out_format!r} must be the layout of the frames, pixel_format={fmt['pixel_format']!r}: the overlay "
                         "is drawn in the format the frames came in, mixed layouts are not supported")
    return True


def _render_out_yuv(frames, out):
    """The tensor a 4:2:0 renderer draws into: a fresh one of the frames' shape unless `out` is given; `out` may be the frames
    themselves (in place) and must otherwise share no memory with them."""
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous")
    if out is None:
        return torch.empty_like(frames)
    if (not torch.is_tensor(out) or out.shape != frames.shape or out.dtype != torch.uint8 or not out.is_contiguous() or
            not out.is_cuda):
        raise ValueError(f"out must be a contiguous uint8 {tuple(frames.shape)} GPU tensor")
    a, b, n = frames.data_ptr(), out.data_ptr(), frames.numel()
    if a != b and a < b + n and b < a + n:
        raise ValueError("out must be the frames themselves (in place) or share no memory with them")
    return out


def _check_rate(sample_rate):
    from .inputs import check_sample_rate
    return check_sample_rate(sample_rate)


def _check_video_wav(wav, sample_rate):
    """predict_video's waveform: floating (n,) at 24 kHz, or with a sample rate floating / int16 (n,) or (C, n)."""
    if sample_rate is None:
        if wav.dim() != 1 or not wav.is_floating_point():
            raise ValueError(f"wav must be a floating (n,) waveform, got {tuple(wav.shape)} {wav.dtype} (a (C, n) waveform needs "
                             "its sample_rate)")
        return
    _check_rate(sample_rate)
    if wav.dim() not in (1, 2) or not (wav.is_floating_point() or wav.dtype == torch.int16):
        raise ValueError(f"with a sample rate wav must be a floating or int16 (n,) or (C, n) waveform, got {tuple(wav.shape)} "
                         f"{wav.dtype}")


class GazePredictor:
    """Gaze prediction with trained weights on one GPU.

    cfg: the model's configuration (NUM_GPUS 1).  checkpoint_path: a ``.pyth`` file, loaded by name and shape
    (checkpoint.load_checkpoint); None falls back to cfg.TEST.CHECKPOINT_FILE_PATH, and with that empty too the weights are the
    random initialisation (a warning says so).  graph=True replays one captured HIP graph per input shape (B, T, S);
    graph=False launches the same kernels eagerly -- the results are the same bit for bit."""

    def __init__(self, cfg, checkpoint_path=None, device=None, graph: bool = True):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise L.CstsError("GazePredictor runs on MI355X only: it needs a GPU device (there is no CPU fallback)")
        if cfg.NUM_GPUS != 1:
            raise ValueError(f"GazePredictor is one process on one GPU: build its cfg with NUM_GPUS 1, got {cfg.NUM_GPUS}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        from .build import build_model
        self.cfg, self.device, self.graph = cfg, device, bool(graph)
        with torch.cuda.device(device):
            self.model = build_model(cfg, gpu_id=device.index)
            if checkpoint_path is None:
                ck.load_test_checkpoint(cfg, self.model)
            else:
                ck.load_checkpoint(checkpoint_path, self.model)
        self.checkpoint_path = checkpoint_path if checkpoint_path is not None else (cfg.TEST.CHECKPOINT_FILE_PATH or None)
        self.model.eval()
        self._steps = {}           # (B, T, S) or (B, T, S, "attention") -> GraphedEvalStep

    @torch.no_grad()
    def predict(self, frames_u8, wav, frames_idx, frame_length, labels=None, attention=False, sample_rate=None, *,
                pixel_format="rgb24", matrix="bt601", full_range=False, window=None):
        """frames_u8 uint8 (B, T, H, W, 3), wav fp32 (B, n) at 24 kHz, frames_idx (B, T) = the sampled frames' positions on the
        clip's time axis of `frame_length` frames -> {"points": (B, T, 2) (x, y) in [0, 1), "peak": (B, T),
        "heatmaps": (B, T, S/4, S/4), "rescaled": same shape} on the device, S = DATA.TEST_CROP_SIZE.
        Frames that come at S x S are normalised as they are; any other size goes through the test-mode spatial sampling (short
        side to S, centre crop: inputs.spatial_sampling(train=False, spatial_idx=1)), so the points are in the crop's
        coordinates.  labels (optional, (B, T, L >= 2) gaze labels): carried through the same crop and returned as "labels".
        attention=True adds the fusion attention maps of predict_batch; the other entries keep their bits.
        sample_rate: None (wav is at 24 kHz: today's path, no extra launch), or the rate wav was recorded at: wav, floating or
        int16, (B, n) or (B, C, n), is first brought to 24 kHz mono on the device (inputs.resample_audio).
        pixel_format "nv12" | "i420" (with matrix "bt601" | "bt709", full_range): frames_u8 is uint8 (B, T, H * 3 / 2, W), 4:2:0
        pictures sampled in place (inputs.spatial_sample); the result is that of the converted RGB frames, bit for bit.
        window (top, left, H, W), 4:2:0 only: the frames are decoder surfaces (B, T, Hs * 3 / 2, Ws) and the pictures their windows
        (inputs.check_window), read in place: the result is that of inputs.yuv_window of the frames, bit for bit."""
        if sample_rate is not None:
            sample_rate = _check_rate(sample_rate)
        for t in (frames_u8, wav, frames_idx) + ((labels,) if labels is not None else ()):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise L.CstsError("GazePredictor runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
        from . import inputs
        H, W, fmt = _picture_hw(frames_u8, 2, pixel_format, matrix, full_range, window)
        B, T = frames_u8.shape[:2]
        if sample_rate is not None:
            if wav.dim() not in (2, 3) or wav.shape[0] != B:
                raise ValueError(f"with a sample rate wav must be ({B}, n) or ({B}, C, n), got {tuple(wav.shape)}")
            with torch.cuda.device(self.device):
                wav = inputs.resample_audio(wav, sample_rate)
        if wav.dim() != 2 or wav.shape[0] != B or tuple(frames_idx.shape) != (B, T):
            raise ValueError(f"wav must be ({B}, n) and frames_idx ({B}, {T}), got {tuple(wav.shape)} and {tuple(frames_idx.shape)}")
        cfg = self.cfg
        S = int(cfg.DATA.TEST_CROP_SIZE)
        mean, std = tuple(cfg.DATA.MEAN), tuple(cfg.DATA.STD)
        with torch.cuda.device(self.device):
            new_labels = labels
            if (H, W) != (S, S):
                lab = labels if labels is not None else torch.zeros(B, T, 2, dtype=torch.float64, device=frames_u8.device)
                video, new_labels = inputs.spatial_sampling(frames_u8, lab, S, train=False, spatial_idx=1, mean=mean, std=std,
                                                            **fmt)
            elif fmt:          # the identity crop of the sampling pass equals normalize_frames of the converted frames bit for bit
                ident = torch.tensor([[S, S, 0, 0, 0]], dtype=torch.int32, device=frames_u8.device).repeat(B, 1)
                video = inputs.spatial_sample(frames_u8, ident, S, mean=mean, std=std, **fmt)
            else:
                video = inputs.normalize_frames(frames_u8, mean=mean, std=std)
            audio = inputs.audio_windows(inputs.stft_logpower(wav), frames_idx, frame_length)
            if S != 256:       # S frequency bins x S columns around each frame, as train.synthetic_batch cuts them
                o = (256 - S) // 2
                audio = audio[:, :, :, :S, o:o + S].contiguous()
            out = self.predict_batch({"video": video, "audio": audio}, attention=attention)
        if labels is not None:
            out["labels"] = new_labels
        return out

    @torch.no_grad()
    def predict_batch(self, batch, attention=False):
        """batch: an assembled dict with "video" fp32 (B, 3, T, S, S) and "audio" fp32 (B, 1, T, F, F) (inputs.assemble_batch,
        train.synthetic_batch) -> the dict of predict().  The tensors are the caller's: a later call does not overwrite them.
        attention=True adds what vis_av_st_fusion of the reference draws (ops.audio_pixel_attn, include/csts_hip.h), with Hh heads
        and the grid (T', h, w) of the spatial fusion block: "audio_attention" (B, Hh, T', h, w) = the probability each image
        region of frame t gives that frame's audio token, "audio_attention_mean" (B, T', h, w) = its head mean, "attention_maps"
        (B, Hh + 1, T, h, w) = one rescaled map per input frame and head (index Hh: the head mean), ready for render_attention,
        "attention_range" (B, Hh + 1, T, 2) = the (lo, hi) each was rescaled by, "temporal_attention" (B, n, n) = the temporal
        fusion block's head-averaged probabilities.  Without the flag the launches are what they were."""
        attention = bool(attention)
        video, audio = batch["video"], batch["audio"]
        for t in (video, audio):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise L.CstsError("GazePredictor runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
        if video.dim() != 5 or audio.dim() != 5:
            raise ValueError(f"video and audio must be 5-D, got {tuple(video.shape)} and {tuple(audio.shape)}")
        with torch.cuda.device(self.device):
            if self.graph:
                key = (video.shape[0], video.shape[2], video.shape[-1]) + (("attention",) if attention else ())
                step = self._steps.get(key)
                if step is None or step.static["audio"].shape != audio.shape or step.static["video"].shape != video.shape:
                    step = self._steps[key] = GraphedEvalStep(self.cfg, self.model, {"video": video, "audio": audio},
                                                              attention=attention)
                out = step.run(video, audio)
                out = {k: out[k].clone() for k in ("points", "peak", "preds", "rescaled") + (tuple(ATTENTION_OUTPUTS) if attention else ())}
            else:
                out = eval_forward(self.model, video.contiguous(), audio.contiguous(), attention=attention)
        res = {"points": out["points"], "peak": out["peak"], "heatmaps": out["preds"].squeeze(1),
               "rescaled": out["rescaled"].squeeze(1)}
        if attention:
            res.update({k: out[k] for k in ATTENTION_OUTPUTS})
        return res

    def stream(self, fps=None, stride=None, segment=None, batch=1, max_chunk=32, pixel_format="rgb24", matrix="bt601",
               full_range=False, sample_rate=None, input_rate=None, live=None, max_gap=None, overlay=False, alpha=0.4, radius=5,
               overlay_format=None, window=None, attention=False, max_age=None, attention_overlay=None):
        """A live stream on this predictor (csts_amd.stream.GazeStream): push(frames, wav) takes frames and 24 kHz audio in whatever
        pieces they arrive and returns the windows each piece completes; close() ends it.  The windows are plan_stream's (fps an
        int or a Fraction, stride in frames); `batch` windows run per predict_batch call; `max_chunk` sizes the two device rings,
        which do not grow with the stream (GazeStream states the capacities).  pixel_format "nv12" | "i420": the pushed frames
        are 4:2:0 pictures; window (top, left, H, W): they are decoder surfaces and the pictures their windows
        (inputs.check_window), H x W the stream's source size; an RGB overlay shows the window, a 4:2:0 one is the surface.
        input_rate=R: the audio is pushed at R Hz, (m,) or (C, m), floating or int16, and resampled to 24 kHz
        mono on the device with the filter state carried from push to push (inputs.StreamResampler): the track of
        inputs.resample_audio on the whole waveform, bit for bit.  sample_rate: None or 24000, the audio as it is; another rate
        there is a ValueError (it keeps no filter state), and so are both keywords together.
        live="hold" | "linear" (forecast plans): push_live(frames, wav) also answers every pushed frame with its row of a gaze
        track computed from the windows that have run by then -- the forecast drawn on the frame it was made for, when that frame
        arrives -- filled at most max_gap frames apart (default: default_max_gap of the plan); overlay=True (needs live) adds
        the frames drawn over with `alpha` and `radius` as render_track takes them.  GazeStream states the causal rule.
        attention=True: every window also carries the fusion attention maps of predict_batch(attention=True)
        (stream.attention_track_from_windows folds them into predict_video(attention_track=True)'s format); with live= every
        pushed frame is also answered with the newest attention map at most max_age frames old (default:
        stream.default_attention_age of the plan), and attention_overlay="mean" | head index (needs overlay=True) adds the
        frames with that map drawn over.  GazeStream states the rule."""
        from .stream import GazeStream
        return GazeStream(self, fps=fps, stride=stride, segment=segment, batch=batch, max_chunk=max_chunk,
                          pixel_format=pixel_format, matrix=matrix, full_range=full_range, sample_rate=sample_rate,
                          input_rate=input_rate, live=live, max_gap=max_gap, overlay=overlay, alpha=alpha, radius=radius,
                          overlay_format=overlay_format, window=window, attention=attention, max_age=max_age,
                          attention_overlay=attention_overlay)

    def stream_group(self, streams, fps=None, stride=None, segment=None, batch=4, max_chunk=32, pixel_format="rgb24",
                     matrix="bt601", full_range=False, input_rate=None, window=None):
        """`streams` live streams on this predictor, served together (csts_amd.stream.GazeStreamGroup): push({slot: (frames,
        wav)}) is one tick -- what all the slots pushed goes into one arena of rings with one launch per stage, and the windows
        that become ready in the same tick are predicted together, `batch` per predict_batch call, whichever slot they belong
        to; close(slot) / close() end a slot / all of them, reset(slot) reopens one.  The keywords are stream()'s and hold for
        every slot; each slot has its own source size.  live=, overlay= and attention are not part of a group (the live
        track of a group is live_group()).  A group takes tight pictures only: a window is a ValueError.  GazeStreamGroup
        states the tick rule and the contract; group_schedule is the rule on the host."""
        from .stream import GazeStreamGroup
        from .inputs import no_window
        no_window(window, "GazeStreamGroup")
        return GazeStreamGroup(self, streams, fps=fps, stride=stride, segment=segment, batch=batch, max_chunk=max_chunk,
                               pixel_format=pixel_format, matrix=matrix, full_range=full_range, input_rate=input_rate)

    def live_group(self, streams, live, fps=None, stride=None, segment=None, batch=4, max_chunk=32, pixel_format="rgb24",
                   matrix="bt601", full_range=False, input_rate=None, max_gap=None, overlay=False, alpha=0.4, radius=5,
                   overlay_format=None, window=None):
        """stream_group() with the live track of stream(live=...) on every slot (csts_amd.stream.GazeLiveGroup, forecast plans):
        push_live({slot: (frames, wav)}) is one tick and returns (windows, {slot: the push_live dict of that slot's frames}) --
        every pushed frame of every slot answered with its row of a gaze track computed from the windows of its own slot that
        have run by then, filled at most max_gap frames apart; overlay=True adds the frames drawn over.  live: "hold" or
        "linear", required.  The tracks of all slots live in one arena and a round folds and answers them with one launch each
        (ops.group_live_add, ops.group_live_rows), whatever the number of slots; their points on the source frames and their
        overlays are one launch each as well, whatever the sizes (ops.group_points_source, ops.group_gaze_overlay).  The other
        keywords are stream_group()'s and stream()'s.  GazeLiveGroup states the order of work and the contract;
        group_live_schedule is the rule on the host.  A window is a ValueError, as in stream_group()."""
        from .stream import GazeLiveGroup
        from .inputs import no_window
        no_window(window, "GazeLiveGroup")
        return GazeLiveGroup(self, streams, live, fps=fps, stride=stride, segment=segment, batch=batch, max_chunk=max_chunk,
                             pixel_format=pixel_format, matrix=matrix, full_range=full_range, input_rate=input_rate,
                             max_gap=max_gap, overlay=overlay, alpha=alpha, radius=radius, overlay_format=overlay_format)

    @torch.no_grad()
    def _video_params_row(self, H, W):
        """The one row of test-mode spatial parameters a whole video is sampled under: (new h, new w, y0, x0, flip)."""
        S = int(self.cfg.DATA.TEST_CROP_SIZE)
        if (H, W) == (S, S):
            return [S, S, 0, 0, 0]                            # identity: bit-equal to normalize_frames
        import numpy as np
        from . import inputs
        T = int(self.cfg.DATA.NUM_FRAMES)
        return inputs.spatial_rule_host(np.zeros((1, T, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()

    @torch.no_grad()
    def render_track(self, frames_u8, track, alpha=0.4, radius=5, out=None, chunk=None, *, pixel_format="rgb24", matrix="bt601",
                     full_range=False, out_format=None, window=None):
        """The track of predict_video drawn onto its recording: frames_u8 uint8 (N, H, W, 3) on the device and the dict
        predict_video returned (it must hold "rescaled" and "points") -> uint8 (N, H, W, 3): the heat map of every predicted
        frame blended over the crop the model saw and a disc at the gaze point (ops.gaze_overlay, csts_gaze_overlay); frames no
        window predicts (NaN points) come back as they are.  The crop is the one predict_video sampled: identity for S x S
        sources, else short side to S and centre crop.  chunk: frames per kernel launch (default: all).  out=frames_u8 renders
        in place.  pixel_format "nv12" | "i420": frames_u8 is the 4:2:0 recording uint8 (N, H * 3 / 2, W); each chunk is converted
        into `out` (inputs.yuv_to_rgb) and drawn over there, so the result is RGB as above and out must not alias the input.
        out_format: None / "rgb24" (the RGB result above), or the frames' own 4:2:0 layout ("nv12" | "i420", equal to
        pixel_format; matrix and range are the input's): the overlay is drawn in that format (ops.gaze_overlay_yuv), the result
        is uint8 (N, H * 3 / 2, W) -- where(drawn, rgb_to_yuv(the RGB result), frames), see include/csts_hip.h -- and
        out=frames_u8 renders in place.  window (top, left, H, W), 4:2:0 only: the frames are decoder surfaces and the pictures
        their windows (the window predict_video was given): the RGB result is (N, H, W, 3) of the window; the 4:2:0 result has the
        surfaces' shape, drawn inside the window and byte for byte the input around it."""
        if not torch.is_tensor(frames_u8) or not frames_u8.is_cuda:
            raise L.CstsError("GazePredictor runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
        if "rescaled" not in track or "points" not in track:
            raise ValueError("render_track needs the track's \"rescaled\" and \"points\": call predict_video with return_heatmaps=True")
        H, W, fmt = _picture_hw(frames_u8, 1, pixel_format, matrix, full_range, window)
        N = frames_u8.shape[0]
        yuv_out = _overlay_yuv(out_format, fmt)
        if yuv_out:
            out = _render_out_yuv(frames_u8, out)
        elif fmt:
            out = _render_out(frames_u8, out, H, W, fmt)
        if track["rescaled"].shape[0] != N or tuple(track["points"].shape) != (N, 2):
            raise ValueError(f"the track holds {track['rescaled'].shape[0]} frames, the recording {N}")
        step = N if chunk is None else int(chunk)
        if step < 1:
            raise ValueError(f"chunk must be positive, got {chunk}")
        S = int(self.cfg.DATA.TEST_CROP_SIZE)
        with torch.cuda.device(self.device):
            row = self._video_params_row(H, W)
            params = torch.tensor(row, dtype=torch.int32, device=frames_u8.device)
            centers = marker_centers(points_to_source(track["points"], row, S), H, W)
            if out is None:
                out = torch.empty_like(frames_u8)
            from . import inputs
            for a in range(0, N, step):
                sel = slice(a, min(a + step, N))
                if yuv_out:
                    ops.gaze_overlay_yuv(frames_u8[sel], track["rescaled"][sel], params, S, centers=centers[sel], alpha=alpha,
                                         radius=radius, out=out[sel], **fmt)
                    continue
                src = inputs.yuv_to_rgb(frames_u8[sel], out=out[sel], **fmt) if fmt else frames_u8[sel]
                ops.gaze_overlay(src, track["rescaled"][sel], params, S, centers=centers[sel], alpha=alpha,
                                 radius=radius, out=out[sel])
        return out

    @torch.no_grad()
    def render_attention(self, frames_u8, result, head=None, alpha=0.4, radius=5, points=None, out=None, *, pixel_format="rgb24",
                         matrix="bt601", full_range=False, out_format=None, window=None):
        """The fusion attention maps of predict(attention=True) drawn onto the clip: frames_u8 uint8 (B, T, H, W, 3) on the device
        (the frames that were predicted) and the result dict (it must hold "attention_maps") -> uint8 (B, T, H, W, 3): the map
        of `head` (None: the head mean) of every input frame blended over the crop the model saw -- one ops.gaze_overlay call
        over the B * T frames.  The crop is predict()'s: identity for S x S frames, else short side to S and centre crop.
        points (optional, (B, T, 2) on the crop, e.g. result["points"]): a disc of `radius` pixels at each (NaN: that frame comes
        back untouched).  out=frames_u8 renders in place.  pixel_format "nv12" | "i420": frames_u8 is uint8 (B, T, H * 3 / 2, W); the
        frames are converted into `out` (inputs.yuv_to_rgb) and drawn over there: out must not alias the input.  out_format: as
        render_track takes it; in the frames' own 4:2:0 layout the result is uint8 (B, T, H * 3 / 2, W) and out=frames_u8 is
        allowed.  window: as render_track takes it (the window predict() was given)."""
        if not torch.is_tensor(frames_u8) or not frames_u8.is_cuda:
            raise L.CstsError("GazePredictor runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
        if "attention_maps" not in result:
            raise ValueError("render_attention needs the result's \"attention_maps\": call predict with attention=True")
        H, W, fmt = _picture_hw(frames_u8, 2, pixel_format, matrix, full_range, window)
        if not frames_u8.is_contiguous():
            raise ValueError("frames must be contiguous")
        B, T = frames_u8.shape[:2]
        maps = result["attention_maps"]
        if maps.dim() != 5 or maps.shape[0] != B or maps.shape[2] != T:
            raise ValueError(f"attention_maps {tuple(maps.shape)} do not belong to {B} clips of {T} frames")
        nheads = maps.shape[1] - 1
        g = nheads if head is None else int(head)
        if head is not None and not 0 <= g < nheads:
            raise ValueError(f"head must be None (the head mean) or lie in [0, {nheads}), got {head!r}")
        yuv_out = _overlay_yuv(out_format, fmt)
        if yuv_out:
            out = _render_out_yuv(frames_u8, out)
        elif fmt:
            out = _render_out(frames_u8, out, H, W, fmt)
        elif out is not None and (out.shape != frames_u8.shape or out.dtype != torch.uint8 or not out.is_contiguous()):
            raise ValueError(f"out must be contiguous uint8 {tuple(frames_u8.shape)}, got {tuple(out.shape)} {out.dtype}")
        S = int(self.cfg.DATA.TEST_CROP_SIZE)
        with torch.cuda.device(self.device):
            row = self._video_params_row(H, W)
            params = torch.tensor(row, dtype=torch.int32, device=frames_u8.device)
            centers = None
            if points is not None:
                if tuple(points.shape) != (B, T, 2):
                    raise ValueError(f"points must be ({B}, {T}, 2), got {tuple(points.shape)}")
                centers = marker_centers(points_to_source(points.reshape(B * T, 2), row, S), H, W)
            if out is None:
                out = torch.empty_like(frames_u8)
            picture = maps[:, g].reshape(B * T, maps.shape[3], maps.shape[4])
            if yuv_out:
                surface = (B * T,) + tuple(frames_u8.shape[2:])
                ops.gaze_overlay_yuv(frames_u8.view(surface), picture, params, S, centers=centers, alpha=alpha, radius=radius,
                                     out=out.view(surface), **fmt)
                return out
            if fmt:
                from . import inputs
                src = inputs.yuv_to_rgb(frames_u8, out=out, **fmt)
            else:
                src = frames_u8
            ops.gaze_overlay(src.view(B * T, H, W, 3), picture, params, S,
                             centers=centers, alpha=alpha, radius=radius, out=out.view(B * T, H, W, 3))
        return out

    @torch.no_grad()
    def render_attention_track(self, frames_u8, track, head=None, alpha=0.4, radius=5, points=None, out=None, chunk=None, *,
                               pixel_format="rgb24", matrix="bt601", full_range=False, out_format=None, window=None):
        """The attention track of predict_video(attention_track=True) drawn onto its recording: frames_u8 uint8 (N, H, W, 3) on
        the device and the track (it must hold "attention_maps" and "attention_count") -> uint8 (N, H, W, 3): on every frame a
        pair landed on, or the fill reached ("attention_filled"), the map of `head` (None: the head mean) blended over the crop
        the model saw -- one ops.gaze_overlay call per chunk.  Every other frame comes back byte for byte.  points (optional,
        (N, 2) on the crop, e.g. the gaze track's "points"): a disc of `radius` pixels where the point is finite; a drawn frame
        without a point gets no disc (its marker centre lies radius + 1 pixels right of the frame).  chunk: frames per launch
        (default: all).  out=frames_u8 renders in place.  pixel_format "nv12" | "i420": frames_u8 is the 4:2:0 recording uint8
        (N, H * 3 / 2, W); each chunk is converted into `out` (inputs.yuv_to_rgb) and drawn over there: out must not alias it.
        out_format: as render_track takes it; in the frames' own 4:2:0 layout the result is uint8 (N, H * 3 / 2, W) and
        out=frames_u8 is allowed.  window: as render_track takes it."""
        if not torch.is_tensor(frames_u8) or not frames_u8.is_cuda:
            raise L.CstsError("GazePredictor runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
        if "attention_maps" not in track or "attention_count" not in track:
            raise ValueError("render_attention_track needs the track's \"attention_maps\" and \"attention_count\": call predict_video "
                             "with attention_track=True")
        H, W, fmt = _picture_hw(frames_u8, 1, pixel_format, matrix, full_range, window)
        N = frames_u8.shape[0]
        yuv_out = _overlay_yuv(out_format, fmt)
        if yuv_out:
            out = _render_out_yuv(frames_u8, out)
        elif fmt:
            out = _render_out(frames_u8, out, H, W, fmt)
        maps, count = track["attention_maps"], track["attention_count"]
        if maps.dim() != 4 or maps.shape[0] != N or tuple(count.shape) != (N,):
            raise ValueError(f"the attention track holds {maps.shape[0]} frames, the recording {N}")
        nheads = maps.shape[1] - 1
        g = nheads if head is None else int(head)
        if head is not None and not 0 <= g < nheads:
            raise ValueError(f"head must be None (the head mean) or lie in [0, {nheads}), got {head!r}")
        if points is not None and tuple(points.shape) != (N, 2):
            raise ValueError(f"points must be ({N}, 2), got {tuple(points.shape)}")
        step = N if chunk is None else int(chunk)
        if step < 1:
            raise ValueError(f"chunk must be positive, got {chunk}")
        radius = int(radius)
        S = int(self.cfg.DATA.TEST_CROP_SIZE)
        with torch.cuda.device(self.device):
            row = self._video_params_row(H, W)
            params = torch.tensor(row, dtype=torch.int32, device=frames_u8.device)
            drawn = count > 0
            if "attention_filled" in track:
                drawn = drawn | track["attention_filled"]
            # drawn, no point: a centre no pixel of the frame is within `radius` of; not drawn: X = -1, the frame passes through
            centers = torch.tensor([W + max(radius, 0) + 1, 0], dtype=torch.int32, device=frames_u8.device).repeat(N, 1)
            if points is not None:
                marks = marker_centers(points_to_source(points, row, S), H, W)
                centers = torch.where(marks[:, :1] >= 0, marks, centers)
            centers = torch.where(drawn[:, None], centers, torch.full_like(centers, -1))
            picture = maps[:, g].contiguous()
            if out is None:
                out = torch.empty_like(frames_u8)
            from . import inputs
            for a in range(0, N, step):
                sel = slice(a, min(a + step, N))
                if yuv_out:
                    ops.gaze_overlay_yuv(frames_u8[sel], picture[sel], params, S, centers=centers[sel], alpha=alpha, radius=radius,
                                         out=out[sel], **fmt)
                    continue
                src = inputs.yuv_to_rgb(frames_u8[sel], out=out[sel], **fmt) if fmt else frames_u8[sel]
                ops.gaze_overlay(src, picture[sel], params, S, centers=centers[sel], alpha=alpha, radius=radius,
                                 out=out[sel])
        return out

    @torch.no_grad()
    def predict_video(self, frames_u8, wav, fps=None, stride=None, batch=None, return_heatmaps=True, overlay=False, fill=None,
                      max_gap=None, attention_track=False, sample_rate=None, *, pixel_format="rgb24", matrix="bt601",
                      full_range=False, overlay_format=None, window=None):
        """A whole recording in, one gaze track out: frames_u8 uint8 (N, H, W, 3) and wav fp32 (n,) at 24 kHz, both resident on
        the device -> {"points": (N, 2), "peak": (N,), "count": (N,) int32 = windows that predicted the frame, "heatmaps" and
        "rescaled": (N, S/4, S/4) (left out with return_heatmaps=False), "windows": their number}, on the device.

        The windows are plan_video's (stride in frames; fps defaults to DATA.TARGET_FPS).  One log-power STFT of the whole
        waveform serves every window; each batch of `batch` windows (default min(TEST.BATCH_SIZE, 8)) is sampled straight out
        of the video (inputs.clip_sample under one row of test-mode spatial parameters: short side to S, centre crop; S x S
        sources are normalised as they are), gets its audio windows (inputs.audio_windows_at) and runs predict_batch.  The last
        batch is filled up by repeating its last window, so one graph shape serves the video; the repeats are dropped.  The
        windows * T heat maps are averaged per video frame and decoded again by ops.gaze_track; frames no window predicts have
        count 0, NaN points and zero maps.  The points are in the crop's coordinates.  overlay=True adds "points_source" (N, 2)
        float64 = the points normalised on the source frame (points_to_source) and "overlay" uint8 (N, H, W, 3) =
        render_track of this track with its defaults.

        fill: None (the sparse track above), "hold" or "linear": the track is fill_track of the sparse one, so every frame
        between two predictions at most max_gap frames apart (default: default_max_gap of the plan, SAMPLING_RATE + 1) carries
        a map and a point; "count" stays, "neighbours" (N, 2) int32, "filled" (N,) bool and "max_gap" (the gap applied, a host
        int) are added, and overlay=True draws the filled track.  Still one forward pass per window.

        attention_track=True: every batch runs predict_batch(attention=True) and one ops.attention_track call over the plan's
        "frames_idx" adds where the audio attends over the recording (include/csts_hip.h, csts_attention_track), with Hh heads on
        the grid (h, w) of the spatial fusion block: "attention_maps" (N, Hh + 1, h, w) = per video frame and head (index Hh: the
        head mean) the mean over the (window, input frame) pairs that show the frame of that pair's time-mixed map, rescaled by
        its own lattice extrema -- render_attention_track draws it; "attention_range" (N, Hh + 1, 2) = those extrema (NaN where
        no pair lands), "attention_mixed" = the mean before the rescale, "attention_count" (N,) int32 = pairs per frame,
        "temporal_attention_windows" (windows, n, n) and "attention_crop_size" (a host int).  A frame one pair shows carries
        predict(attention=True)'s maps of that window and input frame bit for bit.  The track lands on the INPUT frames, the gaze
        track on the predicted ones.  With a fill mode the attention track is filled too (fill_attention_track; default gap
        default_attention_gap of the plan, max_gap overrides it as well): "attention_neighbours", "attention_filled" and
        "attention_max_gap" are added.  Every gaze entry keeps the bits it has without the flag.

        sample_rate: None (wav is at 24 kHz: today's path bit for bit, no extra launch), or the rate the audio was recorded
        at, a positive integer: wav, floating or int16, (n,) or (C, n), is first brought to 24 kHz mono on the device
        (inputs.resample_audio: channel mean, band-limited polyphase resampling), and the result is what this call would give
        for that waveform.  Without a rate a 2-D wav stays an error.

        pixel_format "nv12" | "i420" (with matrix "bt601" | "bt709", full_range): frames_u8 is the 4:2:0 recording uint8
        (N, H * 3 / 2, W), half the bytes of RGB; the windows are sampled straight out of it (inputs.clip_sample in that format,
        no RGB copy of the recording) and every entry equals, bit for bit, that of the converted recording.  "overlay" is
        RGB uint8 (N, H, W, 3) unless overlay_format names the recording's own layout ("nv12" | "i420"; needs overlay=True):
        then it is drawn in that format, uint8 (N, H * 3 / 2, W) (render_track(out_format=...)).

        window (top, left, H, W), 4:2:0 only: frames_u8 holds decoder surfaces (N, Hs * 3 / 2, Ws) -- rows of a pitch Ws, a coded
        height Hs, the chroma behind Hs * Ws bytes -- and the recording is their windows (inputs.check_window), read in place:
        every entry equals that of inputs.yuv_window(frames_u8, ...), bit for bit, and "points_source" is normalised on the
        window's H x W.  An RGB "overlay" is (N, H, W, 3) of the window; a 4:2:0 one has the surfaces' shape and equals the input
        outside the window."""
        if fill not in (None, "hold", "linear"):
            raise ValueError(f"fill must be None, \"hold\" or \"linear\", got {fill!r}")
        if fill is None and max_gap is not None:
            raise ValueError("max_gap belongs to a fill mode: pass fill=\"hold\" or fill=\"linear\"")
        for t in (frames_u8, wav):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise L.CstsError("GazePredictor runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
        from . import inputs
        H, W, fmt = _picture_hw(frames_u8, 1, pixel_format, matrix, full_range, window)
        if overlay_format is not None and not overlay:
            raise ValueError("overlay_format belongs to the overlay: pass overlay=True")
        _overlay_yuv(overlay_format, fmt, "overlay_format")
        _check_video_wav(wav, sample_rate)
        if sample_rate is not None:
            with torch.cuda.device(self.device):
                wav = inputs.resample_audio(wav[None] if wav.dim() == 2 else wav, sample_rate)
                wav = wav[0] if wav.dim() == 2 else wav
        N = frames_u8.shape[0]
        cfg = self.cfg
        S = int(cfg.DATA.TEST_CROP_SIZE)
        T = int(cfg.DATA.NUM_FRAMES)
        mean, std = tuple(cfg.DATA.MEAN), tuple(cfg.DATA.STD)
        nb = min(int(cfg.TEST.BATCH_SIZE), 8) if batch is None else int(batch)
        if nb < 1:
            raise ValueError(f"batch must be positive, got {batch}")
        with torch.cuda.device(self.device):
            dev = frames_u8.device
            spec = inputs.stft_logpower(wav[None])
            plan = plan_video(cfg, N, fps=fps, stride=stride, cols=spec.shape[2])
            nwin = plan["windows"]
            row = self._video_params_row(H, W)
            params = torch.tensor([row], dtype=torch.int32, device=dev).repeat(nb, 1)
            frames_idx = torch.from_numpy(plan["frames_idx"]).to(dev)
            centers = torch.from_numpy(plan["audio_centers"]).to(dev)
            o = (AUDIO_WIDTH - S) // 2
            preds = torch.empty(nwin * T, S // 4, S // 4, dtype=torch.float32, device=dev)
            attention_track = bool(attention_track)
            column = temporal = None
            for w0 in range(0, nwin, nb):
                n = min(nb, nwin - w0)
                sel = slice(w0, w0 + n)
                idx, cen = frames_idx[sel], centers[sel]
                if n < nb:                                    # pad by repeating the last window: one graph shape per video
                    idx = torch.cat([idx, idx[-1:].expand(nb - n, T)])
                    cen = torch.cat([cen, cen[-1:].expand(nb - n, T)])
                video = inputs.clip_sample(frames_u8, idx, params, S, mean=mean, std=std, **fmt)
                audio = inputs.audio_windows_at(spec, cen, AUDIO_WIDTH)
                if S != AUDIO_WIDTH:   # S frequency bins x S columns around each frame, as predict() cuts them
                    audio = audio[:, :, :, :S, o:o + S].contiguous()
                out = self.predict_batch({"video": video, "audio": audio}, attention=attention_track)
                preds[w0 * T:(w0 + n) * T] = out["heatmaps"][:n].reshape(n * T, S // 4, S // 4)
                if attention_track:                           # the padded repeats are dropped here too
                    if column is None:
                        column = torch.empty((nwin,) + tuple(out["audio_attention"].shape[1:]), dtype=torch.float32, device=dev)
                        temporal = torch.empty((nwin,) + tuple(out["temporal_attention"].shape[1:]),
                                               dtype=out["temporal_attention"].dtype, device=dev)
                    column[sel] = out["audio_attention"][:n]
                    temporal[sel] = out["temporal_attention"][:n]
            target = torch.from_numpy(plan["target_idx"].reshape(-1)).to(dev)
            if fill is None:
                want = ("points", "peak", "count") + (("heatmaps", "rescaled") if return_heatmaps or overlay else ())
                track = ops.gaze_track(preds, target, N, want=want)
            else:                                             # the fill reads the sparse maps: they are dropped at the end
                track = fill_track(ops.gaze_track(preds, target, N, want=("heatmaps", "count")), mode=fill, max_gap=max_gap,
                                   plan=plan)
            if attention_track:
                att = ops.attention_track(column, frames_idx, N, T, S)
                track.update({"attention_maps": att["maps"], "attention_range": att["range"], "attention_mixed": att["mixed"],
                              "attention_count": att["count"], "temporal_attention_windows": temporal,
                              "attention_crop_size": S})
                if fill is not None:
                    track = fill_attention_track(track, mode=fill, max_gap=max_gap, plan=plan)
            if overlay:
                track["points_source"] = points_to_source(track["points"], row, S)
                track["overlay"] = self.render_track(frames_u8, track, out_format=overlay_format, **fmt)
            if not return_heatmaps and "heatmaps" in track:
                del track["heatmaps"], track["rescaled"]
        track["windows"] = nwin
        return track
