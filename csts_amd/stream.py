"""Gaze prediction on a live stream: ``plan_video`` without a length, and ``GazeStream``.

``GazePredictor.predict_video`` needs the finished recording resident on the device.  Here the user pushes frames and audio in
whatever pieces they arrive; every window is emitted by the push that completes it, and what the windows read lives in two device
rings (normalised crops, spectrogram columns) whose size does not depend on how long the stream runs.  The host side -- which
window reads which frames and columns, and when it is ready -- is pure arithmetic (``plan_stream``, ``stream_window``,
``stream_schedule``); the device side is the four kernels of csts_amd/csrc/stream.hip behind inputs.stream_stft,
inputs.stream_audio_windows, inputs.stream_ingest and inputs.stream_gather.  With ``live=`` a forecast stream also answers
every pushed frame with its row of a gaze track, out of a third ring (``stream_live_schedule``, ``live_ring_slots``;
ops.live_track_add and ops.live_track_rows, the live-track kernels of stream.hip), and with ``attention=True`` as well with
the newest fusion attention map, out of a fourth (``live_attention_schedule``, ``attention_ring_slots``;
ops.live_attention_add and ops.live_attention_rows, fusion_maps.hip).  ``GazeStreamGroup`` serves several
recordings at once: its slots share one arena of rings, a tick's frames and samples go in with one launch per stage
(inputs.group_stft, inputs.group_ingest) and the windows of different slots that are ready together share a forward;
``group_schedule`` states on the host which windows share a batch.  ``GazeLiveGroup`` adds the live track to a group: the track
rings of all slots share one arena, and a round folds its windows and answers its frames with one launch each
(ops.group_live_add, ops.group_live_rows; ``group_live_schedule`` is the rule on the host); what depends on a slot's own H x W --
the points on the source frame and the overlay -- is one launch each as well, from a job table over slots of different sizes
(ops.group_points_source, ops.group_gaze_overlay; ``infer.overlay_group_table`` is the rule on the host).  What a stream and a
slot of a group do alike on the host is written once, in the functions from ``check_live_args`` to ``live_empty`` that the three
classes call; each class keeps its own device calls and its own allocation timing."""
from __future__ import annotations

import numbers
from fractions import Fraction

from .infer import AUDIO_WIDTH, window_rule
from .inputs import AUDIO_RATE, STFT_HOP, STFT_N_FFT, STFT_WIN

HALF_WIDTH = AUDIO_WIDTH // 2


def check_stream_rate(sample_rate):
    """The sample_rate= of a stream, the rate its audio is pushed at as it is: None or 24000.  Any other rate is a ValueError:
    resampling chunk by chunk needs the filter's state carried from push to push, which sample_rate= does not do; input_rate=
    (inputs.StreamResampler) does."""
    if sample_rate is None:
        return AUDIO_RATE
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, numbers.Integral) or int(sample_rate) != AUDIO_RATE:
        raise ValueError(f"a stream takes its audio at {AUDIO_RATE} Hz, got sample_rate {sample_rate!r}: resampling chunk by chunk "
                         "needs filter state carried between pushes, which sample_rate= does not keep: open the stream with "
                         f"input_rate={sample_rate!r} instead (inputs.StreamResampler carries the state), or use "
                         "predict_video(sample_rate=...) on a finished recording")
    return AUDIO_RATE


def _exact_fps(fps, default):
    """fps as an exact Fraction: an int, a Fraction, or an integral float; anything else is a ValueError."""
    if fps is None:
        fps = default
    if isinstance(fps, bool):
        raise ValueError(f"fps must be an int or a Fraction, got {fps!r}")
    if isinstance(fps, numbers.Integral):
        f = Fraction(int(fps))
    elif isinstance(fps, Fraction):
        f = fps
    elif isinstance(fps, float) and fps == int(fps):
        f = Fraction(int(fps))
    else:
        raise ValueError(f"a stream places its audio windows by the exact ratio of columns to frames: fps must be an int or a "
                         f"fractions.Fraction, e.g. Fraction(30000, 1001), got {fps!r}")
    if f <= 0:
        raise ValueError(f"fps must be positive, got {fps!r}")
    return f


def plan_stream(cfg, fps=None, stride=None, segment=None):
    """plan_video without a length: the window rule of a stream, on the host.

    Returns {"segment", "observed", "stride", "clip_size", "inputs" and "targets" int64 (T,) local to a window's origin} exactly as
    plan_video(cfg, n, fps, stride, segment) has them (infer.window_rule is the one table behind both), plus "fps" and
    "cols_per_frame", both exact fractions.Fraction: cols_per_frame = AUDIO_RATE / (hop * fps) = 200 / fps spectrogram columns per
    video frame.  fps: an int or a Fraction (an integral float is accepted); anything else is a ValueError -- the audio windows of
    an open-ended stream are placed by this ratio alone, so it has to be exact.  fps defaults to DATA.TARGET_FPS.  A ratio that
    leaves the observed span fewer than 257 columns is the error plan_video raises for such a recording."""
    f = _exact_fps(fps, cfg.DATA.TARGET_FPS)
    rule = window_rule(cfg, fps=int(f) if f.denominator == 1 else float(f), stride=stride, segment=segment)
    plan = dict(rule)
    plan["fps"] = f
    plan["cols_per_frame"] = Fraction(AUDIO_RATE, STFT_HOP) / f
    if plan["observed"] * plan["cols_per_frame"] < AUDIO_WIDTH + 1:
        raise ValueError(f"the spectrogram slice of a window has {float(plan['observed'] * plan['cols_per_frame']):.1f} columns "
                         f"({float(plan['cols_per_frame']):.3f} per frame), an audio window needs {AUDIO_WIDTH + 1}")
    return plan


def stream_window(plan, w):
    """Window w of a stream (plan: plan_stream's), o = w * stride:

      frames_idx    = o + inputs, target_idx = o + targets (int64 (T,), absolute frame numbers);
      audio_centers = plan_video's rule with the whole-recording ratio cols / n replaced by rho = cols_per_frame:
                      c0 = floor(o rho), c1 = floor((o + observed) rho), centre = c0 + rint(local / observed * (c1 - c0)) clipped
                      to [c0 + 128, c1 - 1 - 128] (int64 (T,), global column numbers); a slice narrower than 257 columns is the
                      error it is there;
      ready_frames  = o + inputs[-1] + 1: the window needs this many frames pushed;
      ready_samples = hop * (max(audio_centers) + 128): and this many 24 kHz samples -- column f of the STFT reads the samples
                      [120 f - 120, 120 f + 120), so the last column the window reads is final once they are in.

    Where cols * den == num * n for rho = num / den (e.g. 300 frames, 2000 columns, 30 fps) the centres are plan_video's."""
    import numpy as np
    w = int(w)
    if w < 0:
        raise ValueError(f"window numbers start at 0, got {w}")
    rho = plan["cols_per_frame"]
    observed = int(plan["observed"])
    o = w * int(plan["stride"])
    inputs = np.asarray(plan["inputs"], dtype=np.int64)
    c0 = o * rho.numerator // rho.denominator
    c1 = (o + observed) * rho.numerator // rho.denominator
    if c1 - c0 < AUDIO_WIDTH + 1:
        raise ValueError(f"the spectrogram slice of window {w} has {c1 - c0} columns ({float(rho):.3f} per frame), an audio window "
                         f"needs {AUDIO_WIDTH + 1}")
    centers = c0 + np.rint(inputs.astype(np.float64) / observed * (c1 - c0)).astype(np.int64)
    centers = np.clip(centers, c0 + HALF_WIDTH, c1 - 1 - HALF_WIDTH).astype(np.int64)
    return {"window": w, "origin": o, "frames_idx": o + inputs, "target_idx": o + np.asarray(plan["targets"], dtype=np.int64),
            "audio_centers": centers, "first_column": int(c0), "ready_frames": int(o + inputs[-1] + 1),
            "ready_samples": int(STFT_HOP * (int(centers.max()) + HALF_WIDTH))}


def _pushes_at_24k(pushes, input_rate):
    """(frames, samples) counts whose samples are at input_rate -> the same pushes counted in the 24 kHz samples each makes final
    (differences of inputs.resample_ready over the running total; at 24000 Hz, or with input_rate None, they pass through)."""
    if input_rate is None:
        return pushes
    from .inputs import check_sample_rate, resample_ready, resample_rule
    _, up, down, half = resample_rule(check_sample_rate(input_rate, "input_rate"))
    total, converted = 0, []
    for k, m in pushes:
        if int(m) < 0:
            raise ValueError(f"a push holds counts >= 0, got ({k}, {m})")
        before = total
        total += int(m)
        converted.append((k, int(m) if up == down else resample_ready(total, up, down, half) - resample_ready(before, up, down, half)))
    return converted


def stream_schedule(plan, pushes, input_rate=None):
    """Which windows each push completes.  pushes: a list of (frames, samples) counts, one pair per push; returns one list of
    window numbers per push.  Window w is ready in the first push after which ready_frames(w) frames and ready_samples(w) samples
    have been pushed in total; windows are emitted in order, every window once.  input_rate: the sample counts are at that rate,
    as a GazeStream(input_rate=...) takes them; each is first converted to the 24 kHz samples the push makes final (differences
    of inputs.resample_ready over the running total; at 24000 Hz the pieces count as mono fp32, which pass through)."""
    pushes = _pushes_at_24k(pushes, input_rate)
    frames = samples = 0
    w = 0
    nxt = stream_window(plan, 0)
    out = []
    for k, m in pushes:
        k, m = int(k), int(m)
        if k < 0 or m < 0:
            raise ValueError(f"a push holds counts >= 0, got ({k}, {m})")
        frames += k
        samples += m
        ready = []
        while nxt["ready_frames"] <= frames and nxt["ready_samples"] <= samples:
            ready.append(w)
            w += 1
            nxt = stream_window(plan, w)
        out.append(ready)
    return out


def used_frames(plan, a, b):
    """The frames of [a, b) some window reads: f is used iff f - w * stride is one of the plan's inputs for some w >= 0."""
    stride = int(plan["stride"])
    inputs = [int(i) for i in plan["inputs"]]
    return [f for f in range(int(a), int(b)) if any(f >= i and (f - i) % stride == 0 for i in inputs)]


def ring_sizes(plan, max_chunk, crop_size, nbins=STFT_N_FFT // 2 + 1):
    """The two capacities of a GazeStream and their bytes: {"slots": R = observed + max_chunk crops, "crop_bytes": R * 3 * S * S * 4,
    "ring_cols": one observed span of columns plus the audio of max_chunk frames plus the column close() adds, rounded up to a
    multiple of 64, "spec_bytes": nbins * ring_cols * 4}."""
    import math
    rho = plan["cols_per_frame"]
    slots = int(plan["observed"]) + int(max_chunk)
    cols = math.ceil(plan["observed"] * rho) + 1 + math.ceil(int(max_chunk) * rho) + 1
    cols = (cols + 63) // 64 * 64
    S = int(crop_size)
    return {"slots": slots, "crop_bytes": slots * 3 * S * S * 4, "ring_cols": cols, "spec_bytes": int(nbins) * cols * 4}


def ring_limits(nxt, slots, ring_cols):
    """(frames, samples) the two rings take while window `nxt` (a stream_window result) is the oldest one that has not run."""
    frames_max = int(nxt["frames_idx"][0]) + int(slots)                   # frame f overwrites f - R < the window's first input
    cols_max = nxt["first_column"] + int(ring_cols) - 1                   # one column is kept free for close()
    return frames_max, STFT_HOP * cols_max + STFT_HOP - 1


def stream_steps(plan, slots, ring_cols, max_chunk, frames, samples, w, k, m):
    """The steps a push of k frames and m samples is worked off in by a stream that has taken `frames` frames and `samples`
    samples and run the windows below w: [(frames, samples, [windows])], each step being as many samples as the spectrum ring
    takes, at most max_chunk frames as the crop ring takes them, then every window that is ready.  ValueError when neither ring
    can take more and no window is ready.  The one statement of the step rule: GazeStream.push works a push off by it and
    stream_live_schedule replays it."""
    nxt = stream_window(plan, w)
    steps = []
    while True:
        frames_max, samples_max = ring_limits(nxt, slots, ring_cols)
        dm = max(0, min(m, samples_max - samples))
        dk = max(0, min(k, max_chunk, frames_max - frames))
        frames, samples, k, m = frames + dk, samples + dm, k - dk, m - dm
        ready = []
        while nxt["ready_frames"] <= frames and nxt["ready_samples"] <= samples:
            ready.append(w)
            w += 1
            nxt = stream_window(plan, w)
        if dk or dm or ready:
            steps.append((dk, dm, ready))
        if not k and not m:
            return steps
        if not (dk or dm or ready):
            if m:
                raise ValueError(f"the audio runs further ahead of the frames than the spectrum ring holds ({ring_cols} "
                                 f"columns = {ring_cols * STFT_HOP} samples): window {w} still waits for frame "
                                 f"{nxt['ready_frames'] - 1}, {frames} pushed; nothing of this push was consumed")
            raise ValueError(f"the frames run further ahead of the audio than the crop ring holds ({slots} slots): window {w} "
                             f"still waits for sample {nxt['ready_samples'] - 1}, {samples} pushed; nothing of this push was "
                             "consumed")


LIVE_MODES = ("hold", "linear")


def check_live_plan(plan):
    """A live track shows the forecast of a frame when the frame arrives, so every target of a window must lie past the window's
    last input; a plan that predicts frames it has already seen (the estimation configs) is a ValueError."""
    first_target, last_input = int(min(plan["targets"])), int(max(plan["inputs"]))
    if first_target <= last_input:
        raise ValueError(f"live= draws the forecast of a frame when that frame arrives, but this plan predicts frames the window "
                         f"has already seen (its first target is frame {first_target} of the window, its last input frame "
                         f"{last_input}): there is nothing to show on an arriving frame.  Fold the emitted windows with "
                         "track_from_windows (then fill_track / render_track) instead")


def live_ring_slots(plan, max_chunk, max_gap):
    """The capacity Rt of the live track ring (frame t in slot t mod Rt): a ring in which, however the recording is pushed, no
    window's targets recycle a slot some row still reads.

    Take a step after which F frames are in; it pushed dk <= max_chunk of them, frames F - dk .. F - 1, and their rows are
    computed after the step's windows have been added.
      reads   row n looks for neighbours a in [n - max_gap + 1, n) and b in (n, a + max_gap], so it reads frames
              n - max_gap + 1 .. n + max_gap - 1.  The rows of this step and of every later one belong to frames >= F - dk, so the
              lowest frame still read is  L = F - dk - max_gap + 1 >= F - max_chunk - max_gap + 1.
      writes  a window runs once its last input frame is in: o + inputs[-1] + 1 <= F, so the largest target written so far is
              t_max = o + targets[-1] <= F - 1 - inputs[-1] + targets[-1].
    Writing target t recycles the slot of frame t - Rt; that is harmless iff t - Rt < L for every t written before the read:
              F - 1 - inputs[-1] + targets[-1] - Rt < F - max_chunk - max_gap + 1
        <=>   Rt >= (targets[-1] - inputs[-1]) + max_chunk + max_gap - 1.
    Targets ascend with the windows, so a slot never holds a NEWER frame than the one being written, and a row that finds an
    OLDER frame in a slot treats it as empty, which it is: nothing has been predicted for the frame the row asks about.  The
    audio does not enter: a window that waits for audio only runs later, with F larger.  Ego4D forecast plan, max_chunk 32,
    max_gap 9: 64 + 32 + 9 - 1 = 104 slots, 1.7 MB of 64 x 64 sums."""
    check_live_plan(plan)
    max_chunk, max_gap = int(max_chunk), int(max_gap)
    if max_chunk < 1 or max_gap < 1:
        raise ValueError(f"max_chunk and max_gap must be positive, got {max_chunk} and {max_gap}")
    return int(max(plan["targets"])) - int(max(plan["inputs"])) + max_chunk + max_gap - 1


def stream_live_schedule(plan, pushes, max_chunk=32, input_rate=None):
    """The companion of stream_schedule for a live track: known(f) for every frame f of the given pushes, in frame order (a list of
    ints, one per frame).  known(f) is the number of windows that have run when the step that takes frame f in finishes -- the
    steps of stream_steps, which GazeStream.push works a push off by: audio, frames, then the ready windows.  The live row of f
    is computed from windows 0 .. known(f) - 1; every frame of one step has the same known, and known never decreases.  It
    depends on how the recording is pushed: the same frame pushed later, or with more audio, may know more windows.  pushes
    and input_rate as stream_schedule takes them; a push the rings cannot take is the ValueError GazeStream.push raises."""
    sizes = ring_sizes(plan, max_chunk, 1)
    frames = samples = w = 0
    known = []
    for k, m in _pushes_at_24k(pushes, input_rate):
        k, m = int(k), int(m)
        if k < 0 or m < 0:
            raise ValueError(f"a push holds counts >= 0, got ({k}, {m})")
        for dk, dm, ready in stream_steps(plan, sizes["slots"], sizes["ring_cols"], int(max_chunk), frames, samples, w, k, m):
            frames, samples, w = frames + dk, samples + dm, w + len(ready)
            known += [w] * dk
    return known


def track_from_windows(results, n_frames, want=("points", "peak", "count", "heatmaps", "rescaled")):
    """The windows a GazeStream emitted, folded into predict_video's track format by ONE ops.gaze_track call: results (a list of
    push() / close() results, in any grouping) -> {"points" (n_frames, 2), "peak", "count", "heatmaps", "rescaled", ...} as `want`
    names them, plus "windows".  fill_track and render_track work on it unchanged.  Targets at or past n_frames are dropped."""
    import numpy as np
    import torch
    from . import ops
    results = list(results)
    if not results:
        raise ValueError("track_from_windows needs at least one emitted window")
    preds = torch.cat([r["heatmaps"] for r in results], dim=0)
    target = torch.from_numpy(np.concatenate([np.asarray(r["target_idx"], dtype=np.int64) for r in results])).to(preds.device)
    track = ops.gaze_track(preds, target, int(n_frames), want=want)
    track["windows"] = len(results)
    return track


# ---- live attention: the attention track lands on the frames a window SAW, so a live row holds the newest map -----------------------

def default_attention_age(plan):
    """The default max_age of a live attention row: stride - 1 + max(0, observed - 1 - inputs[-1]).

    Push the recording in step, frame n together with its 24000 / fps samples.  Window w (origin o = w * stride) needs frame
    o + inputs[-1], and audio no further than the end of its observed span: its last centre column is at most c1 - 129 with
    c1 = floor((o + observed) * cols_per_frame), so ready_samples < (o + observed) * 24000 / fps, which is in once frame
    o + observed - 1 is.  It therefore runs in the step of a frame r(w) with  o + inputs[-1] <= r(w) <= o + max(inputs[-1],
    observed - 1).  While window w is the last that ran, n <= r(w + 1) - 1, the newest frame with a map is o + inputs[-1] (every
    earlier window ends lower), so a row's age is at most
        r(w + 1) - 1 - (o + inputs[-1]) <= stride - 1 + max(0, observed - 1 - inputs[-1]),
    and every frame from r(0) on finds a map.  Where inputs[-1] == observed - 1 -- both shipped forecast plans -- r(w) is exact,
    frame r(w + 1) - 1 has exactly this age, and no smaller max_age serves: 63 on the Ego4D plan, 39 on the Aria one, stride - 1
    whatever the stride.  (A window whose last input lies before the end of its observed span may run a little earlier than the
    bound says; the default is then safe, not minimal.)"""
    last, observed, stride = int(max(plan["inputs"])), int(plan["observed"]), int(plan["stride"])
    return stride - 1 + max(0, observed - 1 - last)


def attention_ring_slots(plan, max_chunk, max_age):
    """The capacity Ra of the live attention ring (frame t in slot t mod Ra): max(inputs[-1] - inputs[0] - stride + 1,
    max_chunk + max_age), at least 1.  Unlike the targets of the gaze ring, input frames do not ascend from window to window:
    window w + 1's first input lies before window w's last.  Two conditions, both independent of how the recording is pushed:

      a write never meets a NEWER frame in its slot.  Windows run in order and a window's pairs land in ascending frame order.
              Everything written before window w (origin o) is at most o - stride + inputs[-1]; window w writes frames
              >= o + inputs[0].  A write of frame t meets a newer frame t' only if t' = t + k Ra was written before, k >= 1, so
              t' - t <= inputs[-1] - inputs[0] - stride: impossible iff  Ra > inputs[-1] - inputs[0] - stride.  Tight: windows
              w - 1 and w write exactly frames that far apart.  Inside one window a later pair's frame is never lower.
      a restart never recycles a frame some row still reads.  Take a step after which F frames are in; it took dk <= max_chunk
              of them, and their rows are computed after the step's windows have been added.  Row n reads frames n - max_age .. n;
              the rows of this step and of every later one belong to frames >= F - dk, so the lowest frame still read is
              L = F - dk - max_age >= F - max_chunk - max_age.  A window runs once its last input frame is in, so every frame
              written so far is <= F - 1, and writing t recycles t - Ra (and frames further back):
              F - 1 - Ra < F - max_chunk - max_age  <=>  Ra >= max_chunk + max_age.
              A window that runs LATE because its audio lags (the crop ring bounds how late: frames_max of ring_limits) only
              makes F larger for the same writes; the frames it writes lie even further below F - 1.
    The larger bound serves both.  Ego4D forecast plan, max_chunk 32, default max_age 63: max(0, 95) = 95 slots, 95 * 9 * 64
    fp32 = 219 KB of 8 x 8 maps; stride 9, max_age 8: max(55, 40) = 55 slots."""
    max_chunk, max_age = int(max_chunk), int(max_age)
    if max_chunk < 1 or max_age < 0:
        raise ValueError(f"max_chunk must be positive and max_age >= 0, got {max_chunk} and {max_age}")
    spread = int(max(plan["inputs"])) - int(min(plan["inputs"])) - int(plan["stride"])
    return max(1, spread + 1, max_chunk + max_age)


def live_attention_schedule(plan, pushes, max_chunk=32, max_age=None, input_rate=None):
    """The live attention of every frame of the given pushes, on the host: a list of (known, attention_frame), one pair per frame
    in frame order.  known is stream_live_schedule's: the windows that have run when the frame's step finishes.  attention_frame
    is the largest frame in [max(0, n - max_age), n] that is an input frame of one of the windows 0 .. known - 1
    (stream_window's "frames_idx"), -1 when there is none: the frame whose map the live row of n holds.  It follows from
    stream_steps and stream_window alone.  max_age: None takes default_attention_age(plan)."""
    max_age = default_attention_age(plan) if max_age is None else int(max_age)
    if max_age < 0:
        raise ValueError(f"max_age must be >= 0, got {max_age}")
    known = stream_live_schedule(plan, pushes, max_chunk=max_chunk, input_rate=input_rate)
    seen, ran, out = set(), 0, []
    for n, kn in enumerate(known):
        for w in range(ran, kn):
            seen.update(int(f) for f in stream_window(plan, w)["frames_idx"])
        ran = max(ran, kn)
        out.append((kn, next((g for g in range(n, max(0, n - max_age) - 1, -1) if g in seen), -1)))
    return out


def attention_track_from_windows(results, n_frames, crop_size):
    """The windows a GazeStream(attention=True) emitted, folded into predict_video(attention_track=True)'s format by ONE
    ops.attention_track call: results (a list of push() / close() results, in any grouping) -> {"attention_maps",
    "attention_range", "attention_mixed", "attention_count" (infer.ATTENTION_TRACK_KEYS), "temporal_attention_windows" (windows,
    n, n), "attention_crop_size"}.  crop_size: the S of the lattice (DATA.TEST_CROP_SIZE).  fill_attention_track and
    render_attention_track work on it unchanged.  Input frames at or past n_frames are dropped."""
    import numpy as np
    import torch
    from . import ops
    results = list(results)
    if not results:
        raise ValueError("attention_track_from_windows needs at least one emitted window")
    if any("audio_attention" not in r for r in results):
        raise ValueError("attention_track_from_windows needs the windows' \"audio_attention\": open the stream with attention=True")
    column = torch.stack([r["audio_attention"] for r in results], dim=0)
    frames = np.stack([np.asarray(r["frames_idx"], dtype=np.int64) for r in results])
    att = ops.attention_track(column, torch.from_numpy(frames).to(column.device), int(n_frames), frames.shape[1], int(crop_size))
    return {"attention_maps": att["maps"], "attention_range": att["range"], "attention_mixed": att["mixed"],
            "attention_count": att["count"], "temporal_attention_windows": torch.stack([r["temporal_attention"] for r in results]),
            "attention_crop_size": int(crop_size)}


# ---- the host rules of one stream: GazeStream follows them on its scalars, the groups on each slot's entries -------------------------

def _open(s, predictor, fps, stride, segment, max_chunk, pixel_format, matrix, full_range, input_rate, window=None):
    """The fields every stream class derives from its predictor, plan and format arguments, set on `s`: input_rate, fmt,
    predictor, plan, S, T, mean, std, R, ring_cols.  Returns ring_sizes(plan, max_chunk, S).  window: the window of the pushed
    4:2:0 surfaces (GazeStream only); it joins fmt and is checked against the surface when the first frames arrive."""
    from . import inputs
    s.input_rate = None if input_rate is None else inputs.check_sample_rate(input_rate, "input_rate")
    s.fmt = {}
    if inputs.check_pixel_format(pixel_format, matrix, full_range)[0]:
        s.fmt = {"pixel_format": pixel_format, "matrix": matrix, "full_range": bool(full_range)}
    if window is not None:
        s.fmt["window"] = inputs.window_values(pixel_format, window)
    s.predictor = predictor
    cfg = predictor.cfg
    s.plan = plan_stream(cfg, fps=fps, stride=stride, segment=segment)
    s.S, s.T = int(cfg.DATA.TEST_CROP_SIZE), int(cfg.DATA.NUM_FRAMES)
    s.mean, s.std = tuple(cfg.DATA.MEAN), tuple(cfg.DATA.STD)
    sizes = ring_sizes(s.plan, max_chunk, s.S)
    s.R, s.ring_cols = sizes["slots"], sizes["ring_cols"]
    return sizes


def check_live_args(plan, max_chunk, crop_size, fmt, live, max_gap, overlay, alpha, radius, overlay_format, required=False):
    """The live and overlay arguments of a constructor, checked as GazeStream documents them -> (max_gap, overlay_format,
    track_slots, track_bytes), (None, None, 0, 0) without live.  required: live may not be None (a GazeLiveGroup).  fmt: the
    format keywords of the frames, {} for packed RGB.  overlay_format comes back as None unless it names their 4:2:0 layout;
    track_bytes counts the ring's fp32 sums plus a count and a frame tag per slot."""
    from .infer import _overlay_yuv, default_max_gap
    if required and live not in LIVE_MODES:
        raise ValueError(f"live must be one of {LIVE_MODES}, got {live!r}")
    if live is not None and live not in LIVE_MODES:
        raise ValueError(f"live must be None or one of {LIVE_MODES}, got {live!r}")
    if overlay and live is None:
        raise ValueError("overlay=True draws the live track onto the pushed frames: it needs live=\"hold\" or live=\"linear\"")
    if max_gap is not None and live is None:
        raise ValueError("max_gap is the gap the live track fills: it needs live=\"hold\" or live=\"linear\"")
    if overlay_format is not None and not overlay:
        raise ValueError("overlay_format belongs to the overlay: pass overlay=True")
    # the overlay in the pushed frames' own 4:2:0 layout (render_track(out_format=...)) instead of RGB
    overlay_format = overlay_format if _overlay_yuv(overlay_format, fmt, "overlay_format") else None
    if live is None:
        return None, None, 0, 0
    check_live_plan(plan)
    gap = default_max_gap(plan) if max_gap is None else int(max_gap)
    if gap < 1:
        raise ValueError(f"max_gap must be positive, got {max_gap}")
    if not 0.0 <= float(alpha) <= 1.0 or int(radius) < 0:
        raise ValueError(f"alpha must lie in [0, 1] and radius be >= 0, got {alpha} and {radius}")
    track_slots = live_ring_slots(plan, max_chunk, gap)
    side = int(crop_size) // 4                               # the model's heat maps are S/4 x S/4
    return gap, overlay_format, track_slots, track_slots * (side * side * 4 + 4 + 8)


def check_attention_args(cfg, plan, max_chunk, crop_size, live, overlay, attention, max_age, attention_overlay):
    """The attention arguments of GazeStream, checked as it documents them -> (max_age, head, attention_slots, attention_bytes,
    (heads, h, w)); (None, False, 0, 0, None) unless both live and attention are on.  head: the `head` render_attention_track
    takes for attention_overlay ("mean" -> None), False without an attention overlay.  attention_bytes counts the ring's fp32
    sums plus a count and a frame tag per slot."""
    from .infer import attention_grid
    both = live is not None and bool(attention)
    if max_age is not None and not both:
        raise ValueError("max_age is the age up to which a live row holds the newest attention map: it needs live=\"hold\" or "
                         "live=\"linear\" and attention=True")
    if attention_overlay is not None and not both:
        raise ValueError("attention_overlay draws the live attention onto the pushed frames: it needs live=\"hold\" or "
                         "live=\"linear\" and attention=True")
    if attention_overlay is not None and not overlay:
        raise ValueError("attention_overlay belongs to the overlay: pass overlay=True")
    if not both:
        return None, False, 0, 0, None
    age = default_attention_age(plan) if max_age is None else int(max_age)
    if age < 0 or age > 65535:
        raise ValueError(f"max_age must lie in 0..65535, got {max_age}")
    heads, _, h, w = attention_grid(cfg, crop_size)
    head = False
    if attention_overlay is not None:
        if attention_overlay == "mean":
            head = None
        elif isinstance(attention_overlay, bool) or not isinstance(attention_overlay, numbers.Integral) \
                or not 0 <= int(attention_overlay) < heads:
            raise ValueError(f"attention_overlay must be \"mean\" (the head mean) or a head index in [0, {heads}), got {attention_overlay!r}")
        else:
            head = int(attention_overlay)
    slots = attention_ring_slots(plan, max_chunk, age)
    return age, head, slots, slots * ((heads + 1) * h * w * 4 + 4 + 8), (heads, h, w)


def check_piece(who, closed, hw, fmt, resampler, frames, wav):
    """What a push checks and counts of one piece before anything is consumed -> (k, hw, m_in, m): k frames of hw = (H, W) (the
    stream's `hw` when there are no frames), m_in samples as they were pushed, m 24 kHz samples they make final (the
    resampler's check and count, which consume nothing).  A closed stream, an input that is not a GPU tensor (CstsError; `who`
    names the class), a wrong shape or dtype, and an H x W other than the stream's are refused."""
    import torch
    from . import lib as L
    from .infer import _picture_hw
    if closed:
        raise ValueError("the stream is closed: push() after close()")
    for t in (frames, wav):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise L.CstsError(f"{who} runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
    k = m = m_in = 0
    if frames is not None:
        H, W, _ = _picture_hw(frames, 1, fmt.get("pixel_format", "rgb24"), fmt.get("matrix", "bt601"), fmt.get("full_range", False),
                              fmt.get("window"))
        if hw is not None and (H, W) != hw:
            raise ValueError(f"the stream's frames are {hw[0]} x {hw[1]} (fixed by the first push), got {H} x {W}")
        k, hw = frames.shape[0], (H, W)
    if wav is not None and resampler is not None:
        m_in = resampler.check(wav)
        m = resampler.count(m_in, wav)                       # the 24 kHz samples this piece makes final
    elif wav is not None:
        if wav.dim() != 1 or wav.dtype != torch.float32:
            raise ValueError(f"wav must be an fp32 (m,) waveform at {AUDIO_RATE} Hz, got {tuple(wav.shape)} {wav.dtype}")
        m_in = m = wav.numel()
    return k, hw, m_in, m


def audio_tail_step(samples, cols, tail, tail_base, piece, n_total, ring_cols):
    """The audio step of a stream with `samples` 24 kHz samples taken, columns [0, cols) final and the waveform tail `tail` (None
    before the first audio) starting at sample tail_base: take `piece` (1-D, possibly empty) -> (samples, cols, tail, tail_base,
    buf, ranges).  buf = tail + piece, starting at the OLD tail_base, is the buffer to launch on; ranges [(f0, f1)] are the
    columns to compute from it, ascending, each at most one turn of the ring.  Column f is final once sample 120 f + 119 is in;
    n_total >= 0: the signal has ended, the columns are the offline STFT's (csts_stft_frames).  The new tail starts at the first
    sample column `cols` reads; it is a view of buf, which the caller clones so that buf can go."""
    import torch
    buf = piece if tail is None else torch.cat([tail, piece])
    samples += piece.numel()
    final = samples // STFT_HOP
    if n_total >= 0:
        final = max(final, 1 + (samples + 2 * (STFT_N_FFT // 2) - STFT_N_FFT) // STFT_HOP)
    ranges = [(f0, min(f0 + ring_cols, final)) for f0 in range(cols, final, ring_cols)]
    cols = max(cols, final)
    keep = max(0, STFT_HOP * cols + (STFT_N_FFT - STFT_WIN) // 2 - STFT_N_FFT // 2)
    keep = max(keep, tail_base)
    return samples, cols, buf[keep - tail_base:], keep, buf, ranges


def closing_flush(plan, slots, ring_cols, next_window, samples, held):
    """How many of the `held` samples a resampler gives up at close() the spectrum ring still takes (ring_limits)."""
    return max(0, min(held, ring_limits(stream_window(plan, next_window), slots, ring_cols)[1] - samples))


def closing_windows(plan, next_window, frames, cols, started=True):
    """The windows close() runs: from next_window on, every window whose frames are in and whose last audio column lies inside
    the `cols` final columns (the padded last column included).  started: some frame has been pushed."""
    ready, w = [], next_window
    nxt = stream_window(plan, w)
    while started and nxt["ready_frames"] <= frames and int(nxt["audio_centers"].max()) + HALF_WIDTH <= cols:
        ready.append(w)
        w += 1
        nxt = stream_window(plan, w)
    return ready


def dropped_windows(plan, next_window, frames):
    """The windows from next_window on that began -- their first input frame was pushed -- and will not run."""
    w = next_window
    while int(stream_window(plan, w)["frames_idx"][0]) < frames:
        w += 1
    return w - next_window


def pad_rows(rows, batch):
    """A batch of `batch` rows: a short one is padded by repeating its last row, so one graph shape serves every batch."""
    return rows + [rows[-1]] * (batch - len(rows))


def crop_audio(audio, S):
    """S frequency bins x S columns around each frame, as predict_video cuts them (nothing to cut at S = AUDIO_WIDTH)."""
    if S == AUDIO_WIDTH:
        return audio
    o = (AUDIO_WIDTH - S) // 2
    return audio[:, :, :, :S, o:o + S].contiguous()


def window_result(r, out, b, stream=None, attention=False):
    """The dict of one emitted window: r its stream_window, row b of predict_batch's `out`; a group names the slot in "stream".
    attention: also row b of the attention entries of predict_batch(attention=True) (infer.ATTENTION_OUTPUTS)."""
    res = {} if stream is None else {"stream": stream}
    res.update({"window": r["window"], "frames_idx": r["frames_idx"], "target_idx": r["target_idx"], "points": out["points"][b],
                "peak": out["peak"][b], "heatmaps": out["heatmaps"][b], "rescaled": out["rescaled"][b]})
    if attention:
        from .infer import ATTENTION_OUTPUTS
        res.update({k: out[k][b] for k in ATTENTION_OUTPUTS})
    return res


def live_fields(rows, frame_idx, known):
    """What a live answer adds to the rows of ops.live_track_rows / group_live_rows, in place: "filled" (no prediction of its own,
    but neighbours to fill from), "frame_idx" int64 (K,) and "known" int32 (K,), the windows each row was computed from."""
    rows["filled"] = (rows["count"] == 0) & (rows["neighbours"][:, 0] >= 0)
    rows["frame_idx"] = frame_idx
    rows["known"] = known
    return rows


def live_empty(side, device, hw=None, overlay=False, overlay_format=None, surface=None, attention=None, attention_overlay=False):
    """The live dict of a push without frames, K = 0: every field of push_live with its shape and dtype; with overlay the frames'
    shape at the stream's H x W (0 x 0 before the first frame), (0, H * 3 / 2, W) when overlay_format names a 4:2:0 layout --
    (0,) + surface when the stream reads the windows of surfaces of that (Hs * 3 / 2, Ws).  attention: (heads, h, w) of a stream
    with live attention, which adds the six attention entries behind "points_source"; attention_overlay: and the second overlay."""
    import torch
    shapes = {"frame_idx": ((0,), torch.int64), "known": ((0,), torch.int32), "points": ((0, 2), torch.float32),
              "peak": ((0,), torch.float32), "count": ((0,), torch.int32), "neighbours": ((0, 2), torch.int32),
              "filled": ((0,), torch.bool), "rescaled": ((0, side, side), torch.float32),
              "points_source": ((0, 2), torch.float64)}
    if attention is not None:
        heads, h, w = attention
        shapes.update({"attention_frame": ((0,), torch.int64), "attention_count": ((0,), torch.int32),
                       "attention_mixed": ((0, heads + 1, h, w), torch.float32), "attention_maps": ((0, heads + 1, h, w), torch.float32),
                       "attention_range": ((0, heads + 1, 2), torch.float32), "attention_age": ((0,), torch.int64)})
    out = {k: torch.empty(shape, dtype=dt, device=device) for k, (shape, dt) in shapes.items()}
    if overlay:
        H, W = hw if hw is not None else (0, 0)
        shape = ((0,) + tuple(surface) if surface else (0, H * 3 // 2, W)) if overlay_format else (0, H, W, 3)
        out["overlay"] = torch.empty(shape, dtype=torch.uint8, device=device)
        if attention is not None and attention_overlay:
            out["attention_overlay"] = torch.empty(shape, dtype=torch.uint8, device=device)
    return out


def _cat_rows(rows):
    """The live dicts of several steps or rounds as one, in frame order."""
    import torch
    return rows[0] if len(rows) == 1 else {key: torch.cat([r[key] for r in rows], dim=0) for key in rows[0]}


class GazeStream:
    """Gaze prediction while the recording is still running (reach it through GazePredictor.stream).

    push(frames, wav) takes the next frames and the next 24 kHz samples, in pieces of any size and in any proportion, and returns
    the windows that piece completes; close() ends the stream.  With input_rate=R the samples are pushed at R Hz instead, (m,)
    or (C, m), floating or int16, and brought to 24 kHz mono on the device by an inputs.StreamResampler the stream owns: its
    state is carried from push to push, so the 24 kHz track is that of inputs.resample_audio on the whole waveform, bit for bit,
    however it was cut.  `samples` counts the 24 kHz samples taken, `input_samples` the source samples; the resampler holds back
    10 to 30 outputs (at most 1.25 ms) until the inputs they read have arrived, and close() flushes them.

    The windows are plan_stream's: window w starts at frame w * stride, reads the T input frames stream_window names and the audio windows around its centre columns, and runs once both
    have arrived -- through predictor.predict_batch in groups of `batch` (a short group is padded by repeating its last window,
    as predict_video pads, so one graph shape serves the stream).  Each result is a dict: "window" (int), "frames_idx" and
    "target_idx" int64 (T,) numpy, and on the device "points" (T, 2), "peak" (T,), "heatmaps" and "rescaled" (T, S/4, S/4).
    The points are in the crop's coordinates (short side to S, centre crop; S x S sources as they are), as predict_video's.

    Device memory is two rings, neither of which depends on how long the stream runs (ring_sizes; `capacity` holds the numbers):
      crops     fp32 (R, 3, S, S), R = observed + max_chunk slots; frame f lives in slot f mod R.  A frame some window reads is
                resized and normalised ONCE, when it arrives (inputs.stream_ingest); frames no window reads are not touched.
                Ego4D forecast plan, max_chunk 32, S 256: R = 118, 92.8 MB (a 1088 x 1080 source frame is 3.5 MB: 26 frames).
      spectrum  fp32 (256, ring_cols), ring_cols = one observed span of columns + the audio of max_chunk frames + 1, rounded up
                to 64; column f lives at f mod ring_cols.  Ego4D at 30 fps: 832 columns, 852 KB (4.2 s of audio).
    and the waveform tail the unfinished columns still need (fewer than 240 samples) plus the piece being pushed.

    Frames and audio may run ahead of each other by what the rings hold: a push is worked off in steps -- as many samples as the
    spectrum ring takes, at most max_chunk frames as the crop ring takes them, then every window that is ready -- so no slot or
    column is overwritten before the last window that reads it has run, and a push far longer than max_chunk is fine.  When
    neither ring can take more and no window is ready, the push raises a ValueError that names the capacity, BEFORE anything of
    that push is consumed; nothing is ever overwritten silently.  The windows that become ready in one step form that step's groups.

    Difference from predict_video: predict_video scales audio positions by the whole recording's cols / n, which a stream cannot
    know; the stream uses cols_per_frame = 200 / fps, so the centres may differ by a column or two (they agree exactly when
    cols * den == num * n).  Equality with predict_video is therefore not claimed; each window equals, bit for bit, the
    composition clip_sample + stft_logpower + audio_windows_at + predict_batch at stream_window's indices and the same batch
    (with input_rate: stft_logpower of resample_audio of the whole waveform).

    Live track (live="hold" | "linear", forecast plans only): a forecast window predicts frames the camera has not delivered
    yet, so push_live(frames, wav) answers every pushed frame f with its row of a gaze track, and with overlay=True with the
    frame drawn over.  The causal rule: the row is computed from the windows that have run when f's step finishes (audio,
    frames, ready windows, then the rows of the step's frames); with known(f) their number (stream_live_schedule),

      live row of f == row f of fill_track(track_from_windows(results[:known(f)], n_frames=f + max_gap + 1), mode=live, max_gap)

    bit for bit: a predicted frame carries the mean of its maps, added in window order; a frame between two predictions at most
    max_gap apart the earlier map ("hold") or the time-linear blend ("linear"); any other frame is unpredicted (zero maps, NaN
    points, peak 0, count 0, neighbours (-1, -1)).  max_gap defaults to default_max_gap(plan).  The track lives in a third ring,
    fp32 sums (Rt, S/4, S/4) with a count and a frame tag per slot, Rt = live_ring_slots(plan, max_chunk, max_gap) (104 slots,
    1.7 MB on the Ego4D forecast plan): ops.live_track_add folds each step's windows in, ops.live_track_rows reads the rows out.
    What a row knows depends on how the recording is pushed -- a frame pushed in a larger piece, or with more audio, may know one
    window more -- so live rows are reproducible for the same pushes, not across different cuts.  The emitted windows do not
    change by a bit with live on.  An estimation plan (targets inside the observed span) is refused: it has nothing to show on
    an arriving frame.

    Decoder surfaces (window=(top, left, H, W), 4:2:0 formats only): the pushed frames are surfaces uint8 (K, Hs * 3 / 2, Ws) and
    the stream's pictures their windows (inputs.check_window), ingested in place (csts_stream_ingest_yuv_win): H x W is the
    stream's source size, every window and live row equals that of a stream fed inputs.yuv_window of the same pushes, bit for
    bit; an RGB overlay is (K, H, W, 3) of the window, a 4:2:0 overlay has the surfaces' shape and equals them outside the window.

    Attention (attention=True): every window runs predict_batch(attention=True) and its result also carries its rows of
    "audio_attention", "audio_attention_mean", "attention_maps", "attention_range" and "temporal_attention"; the gaze entries
    keep their bits, and attention_track_from_windows folds the emitted windows into predict_video(attention_track=True)'s
    format.  With live= as well, push_live also answers every frame with the fusion attention.  That track lands on the frames a
    window SAW, so when frame n arrives no window that shows n can have run and there are no two neighbours to fill between:
    the live rule is HOLD THE NEWEST MAP.  With A = ops.attention_track(the audio_attention of results[:known(n)], their
    frames_idx, n_frames = n + 1, T, S) and g the largest frame in [max(0, n - max_age), n] with A["count"][g] > 0, the row has
    "attention_frame" = g (-1: none), "attention_count" = A["count"][g] (0), "attention_mixed", "attention_maps" and
    "attention_range" = rows g of A (zero maps and a NaN range without a g) and "attention_age" = n - g (-1), bit for bit for
    the same pushes.  max_age defaults to default_attention_age(plan).  The sums live in a fourth ring, fp32 (Ra, heads + 1, h,
    w) with a count and a frame tag per slot, Ra = attention_ring_slots(plan, max_chunk, max_age) (95 slots, 219 KB on the
    Ego4D forecast plan): ops.live_attention_add folds each step's windows in, ops.live_attention_rows reads the rows out.
    attention_overlay="mean" | head index (needs overlay=True) adds "attention_overlay": render_attention_track of the pushed
    frames with those rows and the gaze rows' points, in the overlay's format; a row without a map comes back byte for byte,
    and "overlay" stays the gaze overlay.  With attention=False nothing changes and no launch is added.

    Out of scope: a delayed display for estimation plans, attention in the stream groups, and equality with predict_video.
    sample_rate= still names the rate the audio is pushed at as it is, 24 kHz only."""

    def __init__(self, predictor, fps=None, stride=None, segment=None, batch=1, max_chunk=32, pixel_format="rgb24",
                 matrix="bt601", full_range=False, sample_rate=None, input_rate=None, live=None, max_gap=None, overlay=False,
                 alpha=0.4, radius=5, overlay_format=None, window=None, attention=False, max_age=None, attention_overlay=None):
        check_stream_rate(sample_rate)
        from . import inputs
        if input_rate is not None and sample_rate is not None:
            raise ValueError(f"sample_rate={sample_rate!r} says the audio is pushed at {AUDIO_RATE} Hz as it is, input_rate="
                             f"{input_rate!r} that it is resampled from that rate: pass one of them")
        self.batch, self.max_chunk = int(batch), int(max_chunk)
        if self.batch < 1 or self.max_chunk < 1:
            raise ValueError(f"batch and max_chunk must be positive, got {batch} and {max_chunk}")
        self.capacity = _open(self, predictor, fps, stride, segment, self.max_chunk, pixel_format, matrix, full_range, input_rate,
                              window)
        self.live, self.overlay, self.alpha, self.radius = live, bool(overlay), float(alpha), int(radius)
        self.max_gap, self.overlay_format, self.track_slots, track_bytes = check_live_args(
            self.plan, self.max_chunk, self.S, self.fmt, live, max_gap, overlay, alpha, radius, overlay_format)
        if live is not None:
            self.capacity = dict(self.capacity, track_slots=self.track_slots, track_bytes=track_bytes)
        self.attention = bool(attention)
        self.max_age, self._attention_head, self.attention_slots, attention_bytes, self._attention_shape = check_attention_args(
            predictor.cfg, self.plan, self.max_chunk, self.S, live, overlay, attention, max_age, attention_overlay)
        if self.attention_slots:
            self.capacity = dict(self.capacity, attention_slots=self.attention_slots, attention_bytes=attention_bytes)
        self.resampler = None if input_rate is None else inputs.StreamResampler(self.input_rate)
        self.input_samples = 0                               # source samples consumed (= samples without input_rate)
        self.frames = self.samples = self.cols = 0          # pushed so far; columns [0, cols) are final
        self.next_window, self.dropped, self.closed = 0, 0, False
        self.hw = self._surface = None                       # H x W of the pictures; (Hs * 3 / 2, Ws) under a window
        self._crops = self._spec = self._tail = self._params = self._track = self._attention_ring = None
        self._tail_base = 0                                  # the stream position of _tail[0]

    # ---- host arithmetic -------------------------------------------------------------------------------------------------------
    def _steps(self, k, m):
        """The steps a push of k frames and m samples is worked off in: [(frames, samples, [windows])]; ValueError when stuck."""
        return stream_steps(self.plan, self.R, self.ring_cols, self.max_chunk, self.frames, self.samples, self.next_window, k, m)

    # ---- device work -----------------------------------------------------------------------------------------------------------
    def _setup(self, H, W, device):
        import torch
        self.hw = (H, W)
        self._params = torch.tensor(self.predictor._video_params_row(H, W), dtype=torch.int32, device=device)
        self._crops = torch.zeros(self.R, 3, self.S, self.S, dtype=torch.float32, device=device)

    def _audio(self, piece, n_total=-1):
        """Take the next samples (a device tensor, possibly empty) and compute the columns they complete."""
        import torch
        from . import inputs
        if self._spec is None:
            self._spec = torch.zeros(STFT_N_FFT // 2 + 1, self.ring_cols, dtype=torch.float32, device=piece.device)
        base = self._tail_base
        self.samples, self.cols, tail, self._tail_base, buf, ranges = audio_tail_step(
            self.samples, self.cols, self._tail, base, piece, n_total, self.ring_cols)
        for f0, f1 in ranges:                                # at most one turn of the ring per launch
            inputs.stream_stft(buf.contiguous(), base, f0, f1, self._spec, n_total=n_total)
        self._tail = tail.clone()

    def _ingest(self, chunk):
        import torch
        from . import inputs
        a = self.frames
        used = used_frames(self.plan, a, a + chunk.shape[0])
        if used:
            pairs = torch.tensor([[f - a, f % self.R] for f in used], dtype=torch.int32, device=chunk.device)
            inputs.stream_ingest(chunk, pairs, self._params, self._crops, mean=self.mean, std=self.std, **self.fmt)
        self.frames += chunk.shape[0]

    def _run(self, windows):
        import numpy as np
        import torch
        from . import inputs
        dev, nb = self._crops.device, self.batch
        results = []
        for g in range(0, len(windows), nb):
            group = [stream_window(self.plan, w) for w in windows[g:g + nb]]
            rows = pad_rows(group, nb)
            slots = np.stack([r["frames_idx"] % self.R for r in rows]).astype(np.int32)
            centers = np.stack([r["audio_centers"] for r in rows]).astype(np.int64)
            video = inputs.stream_gather(self._crops, torch.from_numpy(slots).to(dev))
            audio = inputs.stream_audio_windows(self._spec, self.cols - 1, torch.from_numpy(centers).to(dev), centers, AUDIO_WIDTH)
            batch = {"video": video, "audio": crop_audio(audio, self.S)}
            out = self.predictor.predict_batch(batch, attention=True) if self.attention else self.predictor.predict_batch(batch)
            results += [window_result(r, out, i, attention=self.attention) for i, r in enumerate(group)]
        self.next_window = windows[-1] + 1
        return results

    # ---- the interface ---------------------------------------------------------------------------------------------------------
    def push(self, frames=None, wav=None):
        """The next frames -- uint8 (K, H, W, 3), or (K, H * 3 / 2, W) in the stream's pixel format -- and / or the next samples --
        fp32 (m,) at 24 kHz, or with input_rate (m,) / (C, m), floating or int16, at that rate -- both on the device -> the list
        (possibly empty) of the windows this push completes, in order.  On a live stream the windows are folded into the track
        ring as well, so push and push_live may be mixed; a frame is only answered by the push_live that takes it in."""
        return self._push(frames, wav, False)[0]

    def push_live(self, frames=None, wav=None):
        """push() on a stream opened with live=: -> (windows, live).  windows is what push returns.  live answers the K frames of
        this push, in order, on the device: "frame_idx" int64 (K,), "known" int32 (K,) = the windows the row was computed from
        (stream_live_schedule), "points" (K, 2) on the crop, "peak" (K,), "count" int32 (K,), "neighbours" int32 (K, 2), "filled"
        bool (K,), "rescaled" (K, S/4, S/4), "points_source" float64 (K, 2) on the source frame, and with overlay=True "overlay"
        uint8 (K, H, W, 3), the frames drawn over as render_track draws a track (an unpredicted frame comes back as it is).  A
        push longer than max_chunk is worked off in steps and its rows are concatenated; a push without frames has K = 0."""
        if self.live is None:
            raise ValueError("push_live answers frames with the live track: open the stream with live=\"hold\" or live=\"linear\"")
        return self._push(frames, wav, True)

    def _live_add(self, results, f_start):
        """Fold the windows a step ran into the track ring; f_start: the first frame whose row is still to come."""
        import numpy as np
        import torch
        from . import ops
        maps = torch.cat([r["heatmaps"] for r in results], dim=0)
        if self._track is None:
            self._track = ops.live_track_ring(self.track_slots, maps.shape[1], maps.shape[2], maps.device)
        targets = np.concatenate([np.asarray(r["target_idx"], dtype=np.int64) for r in results])
        ops.live_track_add(maps, torch.from_numpy(targets).to(maps.device), targets, self._track,
                           live_from=max(0, f_start - self.max_gap + 1))
        if self.attention:
            column = torch.stack([r["audio_attention"] for r in results], dim=0)
            frames = np.stack([np.asarray(r["frames_idx"], dtype=np.int64) for r in results])
            ops.live_attention_add(column, torch.from_numpy(frames).to(column.device), frames, self._attention(column.device),
                                   live_from=max(0, f_start - self.max_age))

    def _attention(self, device):
        """The attention ring, allocated when the first window is folded in or the first row asked for."""
        from . import ops
        if self._attention_ring is None:
            self._attention_ring = ops.live_attention_ring(self.attention_slots, *self._attention_shape, device)
        return self._attention_ring

    def _live_rows(self, f0, chunk):
        """The live rows of the step's frames f0 .. f0 + K - 1 (chunk: those frames as they were pushed)."""
        import torch
        from . import ops
        from .infer import points_to_source
        K, dev = chunk.shape[0], chunk.device
        if self._track is None:                              # no window has run yet: every row is the unpredicted one
            side = self.S // 4
            self._track = ops.live_track_ring(self.track_slots, side, side, dev)
        rows = ops.live_track_rows(self._track, f0, K, mode=self.live, max_gap=self.max_gap,
                                   want=("rescaled", "points", "peak", "count", "neighbours"))
        live_fields(rows, torch.arange(f0, f0 + K, dtype=torch.int64, device=dev),
                    torch.full((K,), self.next_window, dtype=torch.int32, device=dev))
        rows["points_source"] = points_to_source(rows["points"], self.predictor._video_params_row(*self.hw), self.S)
        if self.attention:
            att = ops.live_attention_rows(self._attention(dev), f0, K, self.S, self.max_age)
            rows.update({"attention_" + k: att[k] for k in ("frame", "count", "mixed", "maps", "range")})
            rows["attention_age"] = torch.where(att["frame"] >= 0, rows["frame_idx"] - att["frame"], torch.full_like(att["frame"], -1))
        if self.overlay:
            rows["overlay"] = self.predictor.render_track(chunk, rows, alpha=self.alpha, radius=self.radius,
                                                          out_format=self.overlay_format, **self.fmt)
            if self._attention_head is not False:
                rows["attention_overlay"] = self.predictor.render_attention_track(
                    chunk, rows, head=self._attention_head, alpha=self.alpha, radius=self.radius, points=rows["points"],
                    out_format=self.overlay_format, **self.fmt)
        return rows

    def _push(self, frames, wav, want_live):
        import torch
        k, hw, m_in, m = check_piece("GazeStream", self.closed, self.hw, self.fmt, self.resampler, frames, wav)
        steps = self._steps(k, m)                            # raises before anything is consumed, the resampler included
        results, rows = [], []
        fa = sa = 0
        with torch.no_grad(), torch.cuda.device(self.predictor.device):
            if k and self.hw is None:
                self._setup(*hw, frames.device)
                self._surface = tuple(frames.shape[1:]) if "window" in self.fmt else None
            if wav is not None:
                self.input_samples += m_in
                if self.resampler is not None:
                    wav = self.resampler.push(wav)           # the whole piece once; the steps slice the 24 kHz samples
            for dk, dm, ready in steps:
                if dm:
                    self._audio(wav[sa:sa + dm])
                    sa += dm
                if dk:
                    self._ingest(frames[fa:fa + dk])
                    fa += dk
                if ready:
                    ran = self._run(ready)
                    results += ran
                    if self.live is not None:                # before the rows of this step's frames, which come last
                        self._live_add(ran, self.frames - dk)
                if dk and want_live:
                    rows.append(self._live_rows(self.frames - dk, frames[fa - dk:fa]))
            if not want_live:
                return results, None
            if not rows:
                dev = frames.device if frames is not None else (wav.device if wav is not None else self.predictor.device)
                return results, live_empty(self.S // 4, dev, self.hw, self.overlay, self.overlay_format, self._surface,
                                           attention=self._attention_shape, attention_overlay=self._attention_head is not False)
            live = _cat_rows(rows)
        return results, live

    def close(self, wav_pad=True):
        """End the stream.  wav_pad: the column the offline STFT adds at the end of a waveform whose length is no multiple of the
        hop -- zeros past the last sample -- is computed, and the windows it completes are returned.  Windows that began (their
        first input frame was pushed) but still miss frames or audio are dropped and counted in `dropped`.  After close(), push()
        is an error."""
        import torch
        if self.closed:
            raise ValueError("the stream is closed already")
        self.closed = True
        results = []
        with torch.no_grad(), torch.cuda.device(self.predictor.device):
            if self.resampler is not None:                   # the outputs held back; as many of them as the spectrum ring takes
                rest = self.resampler.close()
                rest = rest[:closing_flush(self.plan, self.R, self.ring_cols, self.next_window, self.samples, rest.numel())]
                if rest.numel():
                    self._audio(rest)
            if wav_pad and self._tail is not None:
                self._audio(self._tail[:0], n_total=self.samples)
            ready = closing_windows(self.plan, self.next_window, self.frames, self.cols, started=self._crops is not None)
            if ready:
                results = self._run(ready)
        self.dropped += dropped_windows(self.plan, self.next_window, self.frames)
        return results


# ---- stream group: N streams on one predictor, their windows batched together -------------------------------------------------------

def _tick_rounds(steps, batch):
    """The rounds of one tick.  steps: {slot: that slot's stream_steps}.  Round r takes step r of every slot that has one, in slot
    order; its ready windows over all slots, ordered by (slot, window), are cut into consecutive groups of `batch`.  Returns
    [({slot: (frames, samples, [windows])}, [[(slot, window), ...], ...])], one pair per round.  The one statement of the tick
    rule: GazeStreamGroup.push works a tick off by it and group_schedule replays it."""
    rounds = []
    for r in range(max((len(s) for s in steps.values()), default=0)):
        part = {i: steps[i][r] for i in sorted(steps) if r < len(steps[i])}
        rows = [(i, w) for i, (_, _, ready) in part.items() for w in ready]
        rounds.append((part, [rows[g:g + batch] for g in range(0, len(rows), batch)]))
    return rounds


def group_schedule(plan, ticks, batch, max_chunk=32, input_rate=None):
    """The batches a GazeStreamGroup runs, on the host.  ticks: a list of {slot: (frames, samples)} counts, one dict per
    GazeStreamGroup.push; returns, per tick, the list of its batches, each a list of (slot, window) pairs in the order of the
    batch's rows (a batch shorter than `batch` is padded by repeating its last row when it runs).

    One tick: every slot's steps are computed by stream_steps on that slot's counters, in slot order, before anything is
    consumed; a slot that is stuck raises stream_steps' ValueError prefixed with "slot i: " and nothing of the tick counts for
    any slot.  Then the tick runs in rounds: round r takes step r of every slot that has one -- their samples, then their
    frames, then the windows that are ready, ordered by (slot, window) and cut into consecutive groups of `batch`.  Batches
    never mix rounds.  input_rate: the sample counts are at that rate, as stream_schedule takes them."""
    batch, max_chunk = int(batch), int(max_chunk)
    if batch < 1 or max_chunk < 1:
        raise ValueError(f"batch and max_chunk must be positive, got {batch} and {max_chunk}")
    sizes = ring_sizes(plan, max_chunk, 1)
    ratio = None
    if input_rate is not None:
        from .inputs import check_sample_rate, resample_ready, resample_rule
        _, up, down, half = resample_rule(check_sample_rate(input_rate, "input_rate"))
        ratio = None if up == down else (up, down, half)
    state, out = {}, []                                      # slot -> (frames, 24 kHz samples, next window, source samples)
    for tick in ticks:
        steps, after = {}, {}
        for i in sorted(tick):
            k, m = (int(v) for v in tick[i])
            if k < 0 or m < 0:
                raise ValueError(f"slot {i}: a push holds counts >= 0, got ({k}, {m})")
            frames, samples, w, source = state.get(i, (0, 0, 0, 0))
            m24 = m if ratio is None else resample_ready(source + m, *ratio) - resample_ready(source, *ratio)
            try:
                steps[i] = stream_steps(plan, sizes["slots"], sizes["ring_cols"], max_chunk, frames, samples, w, k, m24)
            except ValueError as e:
                raise ValueError(f"slot {i}: {e}") from None
            after[i] = (frames + k, samples + m24, w + sum(len(ready) for _, _, ready in steps[i]), source + m)
        state.update(after)
        out.append([rows for _, batches in _tick_rounds(steps, batch) for rows in batches])
    return out


class GazeStreamGroup:
    """Several live streams on one predictor, their windows predicted together (reach it through GazePredictor.stream_group).

    `streams` slots, each one recording: its own source size H x W, fixed by its first push, and its own counters, the lists
    `frames`, `samples`, `input_samples`, `cols`, `next_window`, `dropped`, `closed`, one entry per slot, as a GazeStream has
    them; `batches` holds the batches the last push() or close() ran, as group_schedule lists them.  All slots share one plan (plan_stream), one pixel format, matrix and range, and one input_rate.

    push(pieces) is one TICK: pieces is {slot: (frames or None, wav or None)} -- or a list of (slot, frames, wav) with distinct
    slots -- with frames and samples as GazeStream.push takes them, and the answer is {slot: [window dicts]} for the slots of
    pieces, each dict a GazeStream result plus "stream": slot.  A tick is worked off by the rule group_schedule states:
      1. every slot's steps are computed by stream_steps on that slot's counters, in slot order, before anything is consumed
         (the resampler's check / count included);
      2. a slot that is stuck, or any input that is invalid (wrong device, wrong shape, H x W differing from the slot's, a closed
         slot) raises the ValueError / CstsError GazeStream raises, prefixed with "slot i: ", and nothing of the tick is consumed
         for any slot;
      3. the tick runs in rounds; round r takes step r of every slot that has one: all their samples go in with ONE STFT launch
         (inputs.group_stft), then all their frames with ONE ingest launch (inputs.group_ingest), then the ready windows of the
         round over all slots, ordered by (slot, window), are cut into consecutive groups of `batch`, the last one padded by
         repeating its last row; each group is one predict_batch call, so one graph shape serves the group;
      4. a round's windows run before the next round's ingest, so no slot or column is overwritten before its last reader has
         run: GazeStream's argument, per slot.

    Device memory is two arenas, allocated once, when the group is made (a GazeStream allocates its spectrum ring on the first
    audio; here both are there from the start): crops fp32 (streams, R, 3, S, S) and spectrum fp32 (streams, 256, ring_cols),
    R and ring_cols from ring_sizes(plan, max_chunk, S), so a slot's ring is exactly a GazeStream's.  `capacity` holds the
    per-slot numbers, "streams" and "total_bytes".

    close(slot) ends one slot as GazeStream.close(wav_pad=True) does -- the resampler is flushed, the padded last column computed,
    the windows that completes run, the begun-but-incomplete ones counted in dropped[slot]; close() does so for every open slot and
    batches the last windows of all of them together in (slot, window) order.  Both return {slot: [window dicts]}.  reset(slot)
    reopens a closed slot as a fresh stream: counters zero, H x W free again, a fresh resampler.  It writes nothing to the
    rings: an audio window is NaN unless it lies inside the columns the slot's new counters have written, and a window runs only
    after every frame it reads has been ingested over what the slots held.

    The contract: every emitted window equals, bit for bit, its row of predict_batch on the batch group_schedule names, each row
    of which is built from that slot's own whole recording by clip_sample at stream_window's frames and audio_windows_at on
    stft_logpower of its whole waveform (with input_rate: of resample_audio of the whole waveform).  A group of one slot equals
    a GazeStream with the same batch, bit for bit.  Nothing is claimed about a row's bits when its batch neighbours change.

    Not accepted as keywords here: live= and overlay=.  The live track of a group is GazeLiveGroup, a subclass (reach it through
    GazePredictor.live_group).  Out of scope: attention maps; different plans per slot; equality with predict_video."""

    def __init__(self, predictor, streams, fps=None, stride=None, segment=None, batch=4, max_chunk=32, pixel_format="rgb24",
                 matrix="bt601", full_range=False, input_rate=None, window=None):
        import torch
        from . import inputs
        inputs.no_window(window, type(self).__name__)        # the grouped kernels take tight pictures only
        self.streams, self.batch, self.max_chunk = int(streams), int(batch), int(max_chunk)
        if self.streams < 1 or self.batch < 1 or self.max_chunk < 1:
            raise ValueError(f"streams, batch and max_chunk must be positive, got {streams}, {batch} and {max_chunk}")
        sizes = _open(self, predictor, fps, stride, segment, self.max_chunk, pixel_format, matrix, full_range, input_rate)
        self.capacity = dict(sizes, streams=self.streams, total_bytes=self.streams * (sizes["crop_bytes"] + sizes["spec_bytes"]))
        n = self.streams
        self.frames, self.samples, self.input_samples, self.cols = [0] * n, [0] * n, [0] * n, [0] * n
        self.next_window, self.dropped, self.closed, self.hw = [0] * n, [0] * n, [False] * n, [None] * n
        self._rows, self._tail, self._tail_base = [None] * n, [None] * n, [0] * n
        self._resamplers = [None if input_rate is None else inputs.StreamResampler(self.input_rate) for _ in range(n)]
        self.batches = []                                    # the batches the last push() / close() ran: [[(slot, window), ...]]
        self._crops = torch.zeros(n, self.R, 3, self.S, self.S, dtype=torch.float32, device=predictor.device)
        self._spec = torch.zeros(n, STFT_N_FFT // 2 + 1, self.ring_cols, dtype=torch.float32, device=predictor.device)

    # ---- host arithmetic -------------------------------------------------------------------------------------------------------
    def _slot(self, slot):
        if isinstance(slot, bool) or not isinstance(slot, numbers.Integral) or not 0 <= int(slot) < self.streams:
            raise ValueError(f"a slot is an integer in [0, {self.streams}), got {slot!r}")
        return int(slot)

    def _plan_slot(self, i, frames, wav):
        """What GazeStream._push checks and counts before it consumes anything, on slot i: (k, (H, W), m_in, m, steps)."""
        k, hw, m_in, m = check_piece("GazeStreamGroup", self.closed[i], self.hw[i], self.fmt, self._resamplers[i], frames, wav)
        steps = stream_steps(self.plan, self.R, self.ring_cols, self.max_chunk, self.frames[i], self.samples[i],
                             self.next_window[i], k, m)
        return k, hw, m_in, m, steps

    # ---- device work -----------------------------------------------------------------------------------------------------------
    def _audio(self, jobs):
        """jobs: [(slot, the next samples of that slot, n_total)], distinct slots: the columns they complete, in one launch."""
        from . import inputs
        pending = []
        for i, piece, n_total in jobs:
            base = self._tail_base[i]
            self.samples[i], self.cols[i], tail, self._tail_base[i], buf, ranges = audio_tail_step(
                self.samples[i], self.cols[i], self._tail[i], base, piece, n_total, self.ring_cols)
            pending.append((buf.contiguous(), base, ranges, i, n_total))
            self._tail[i] = tail.clone()
        for t in range(max((len(p[2]) for p in pending), default=0)):       # at most one turn of a ring per launch
            inputs.group_stft([(buf, base, *ranges[t], i, n_total) for buf, base, ranges, i, n_total in pending if t < len(ranges)],
                              self._spec)

    def _ingest(self, jobs):
        """jobs: [(slot, the next frames of that slot)]: the frames of them some window reads, sampled in one launch."""
        from . import inputs
        table, pairs = [], []
        for i, chunk in jobs:
            a = self.frames[i]
            used = used_frames(self.plan, a, a + chunk.shape[0])
            if used:
                pairs += [(len(table), f - a, i * self.R + f % self.R) for f in used]
                table.append((chunk, self._rows[i]))
            self.frames[i] += chunk.shape[0]
        if pairs:
            inputs.group_ingest(table, pairs, self._crops.view(-1, 3, self.S, self.S), mean=self.mean, std=self.std, **self.fmt)

    def _run(self, rows):
        """One batch: rows [(slot, window)], at most `batch` of them, padded by repeating the last."""
        import numpy as np
        import torch
        from . import inputs
        S = self.S
        self.batches.append(list(rows))
        group = [(i, stream_window(self.plan, w)) for i, w in rows]
        padded = pad_rows(group, self.batch)
        slots = np.stack([i * self.R + r["frames_idx"] % self.R for i, r in padded]).astype(np.int32)
        centers = np.stack([r["audio_centers"] for _, r in padded]).astype(np.int64)
        video = inputs.stream_gather(self._crops.view(-1, 3, S, S), torch.from_numpy(slots).to(self._crops.device))
        audio = inputs.group_audio_windows(self._spec, [i for i, _ in padded], [c - 1 for c in self.cols], centers, AUDIO_WIDTH)
        out = self.predictor.predict_batch({"video": video, "audio": crop_audio(audio, S)})
        for i, r in group:
            self.next_window[i] = r["window"] + 1
        return [window_result(r, out, b, stream=i) for b, (i, r) in enumerate(group)]

    # ---- the interface ---------------------------------------------------------------------------------------------------------
    def push(self, pieces):
        """One tick: {slot: (frames or None, wav or None)}, or a list of (slot, frames, wav) with distinct slots -> {slot: [the
        windows this tick completes for that slot, in order]} for the slots of pieces."""
        import torch
        from . import lib as L
        items = [(i, *v) for i, v in pieces.items()] if isinstance(pieces, dict) else [tuple(p) for p in pieces]
        if any(len(p) != 3 for p in items):
            raise ValueError("a piece is (frames or None, wav or None) under its slot, or (slot, frames, wav) in a list")
        items = sorted(((self._slot(i), frames, wav) for i, frames, wav in items), key=lambda p: p[0])
        if len({p[0] for p in items}) != len(items):
            raise ValueError(f"a tick names every slot at most once, got {[p[0] for p in items]}")
        planned = {}
        for i, frames, wav in items:                         # everything that can refuse the tick, before anything is consumed
            try:
                planned[i] = self._plan_slot(i, frames, wav)
            except L.CstsError as e:
                raise L.CstsError(f"slot {i}: {e}") from None
            except ValueError as e:
                raise ValueError(f"slot {i}: {e}") from None
        self.batches = []
        out = {i: [] for i, _, _ in items}
        given = {i: [frames, wav] for i, frames, wav in items}
        fa, sa = dict.fromkeys(out, 0), dict.fromkeys(out, 0)
        with torch.no_grad(), torch.cuda.device(self.predictor.device):
            for i, (k, hw, m_in, _, _) in planned.items():
                if k and self.hw[i] is None:
                    self.hw[i], self._rows[i] = hw, self.predictor._video_params_row(*hw)
                if given[i][1] is not None:
                    self.input_samples[i] += m_in
                    if self._resamplers[i] is not None:      # the whole piece once; the rounds slice the 24 kHz samples
                        given[i][1] = self._resamplers[i].push(given[i][1])
            for part, batches in _tick_rounds({i: p[4] for i, p in planned.items()}, self.batch):
                self._audio([(i, given[i][1][sa[i]:sa[i] + dm], -1) for i, (_, dm, _) in part.items() if dm])
                chunks = [(i, given[i][0][fa[i]:fa[i] + dk]) for i, (dk, _, _) in part.items() if dk]
                self._ingest(chunks)
                for i, (dk, dm, _) in part.items():
                    fa[i], sa[i] = fa[i] + dk, sa[i] + dm
                ran = []
                for rows in batches:
                    ran += self._run(rows)
                for r in ran:
                    out[r["stream"]].append(r)
                self._round_done(ran, chunks)
        return out

    def _round_done(self, ran, chunks):
        """The end of a round of push(): `ran`, the windows the round ran over all slots in (slot, window) order, and `chunks`,
        [(slot, the frames that slot took in this round)] in slot order.  Nothing here; GazeLiveGroup folds and answers."""

    def close(self, slot=None):
        """End slot `slot`, or with None every slot that is still open -> {slot: [the windows the padded last column completes]}.
        The closing windows of all the slots are batched together, ordered by (slot, window)."""
        import torch
        slots = [i for i in range(self.streams) if not self.closed[i]] if slot is None else [self._slot(slot)]
        if slot is not None and self.closed[slots[0]]:
            raise ValueError(f"slot {slots[0]}: the stream is closed already")
        self.batches = []
        out = {i: [] for i in slots}
        with torch.no_grad(), torch.cuda.device(self.predictor.device):
            flush = []
            for i in slots:
                self.closed[i] = True
                if self._resamplers[i] is not None:          # the outputs held back; as many of them as the spectrum ring takes
                    rest = self._resamplers[i].close()
                    rest = rest[:closing_flush(self.plan, self.R, self.ring_cols, self.next_window[i], self.samples[i], rest.numel())]
                    if rest.numel():
                        flush.append((i, rest, -1))
            self._audio(flush)
            self._audio([(i, self._tail[i][:0], self.samples[i]) for i in slots if self._tail[i] is not None])
            rows = [(i, w) for i in slots for w in closing_windows(self.plan, self.next_window[i], self.frames[i], self.cols[i],
                                                                   started=self.hw[i] is not None)]
            for g in range(0, len(rows), self.batch):
                for r in self._run(rows[g:g + self.batch]):
                    out[r["stream"]].append(r)
        for i in slots:
            self.dropped[i] += dropped_windows(self.plan, self.next_window[i], self.frames[i])
        return out

    def reset(self, slot):
        """Reopen the closed slot `slot` as a fresh stream.  Nothing is written to the rings."""
        from . import inputs
        i = self._slot(slot)
        if not self.closed[i]:
            raise ValueError(f"slot {i}: reset() reopens a closed slot; close({i}) first")
        self.frames[i] = self.samples[i] = self.input_samples[i] = self.cols[i] = self.next_window[i] = self.dropped[i] = 0
        self.closed[i], self.hw[i], self._rows[i], self._tail[i], self._tail_base[i] = False, None, None, None, 0
        if self.input_rate is not None:
            self._resamplers[i] = inputs.StreamResampler(self.input_rate)


# ---- live group: the live track of GazeStream on every slot of a group ----------------------------------------------------------------

def group_live_schedule(plan, ticks, max_chunk=32, input_rate=None):
    """The companion of group_schedule for a GazeLiveGroup: {slot: [known(f) for every frame f that slot pushed, in frame order]}.
    ticks: a list of {slot: (frames, samples)} counts, one dict per push, as group_schedule takes them.  Round r of a tick takes
    step r of every slot, and a slot's steps come from stream_steps on that slot's own counters, so what a frame knows does not
    depend on the other slots: this is stream_live_schedule on each slot's own pushes, and it is computed as that.  A slot that
    is stuck raises stream_steps' ValueError prefixed with "slot i: ", as group_schedule does."""
    pushes = {}
    for tick in ticks:
        for i in sorted(tick):
            k, m = (int(v) for v in tick[i])
            pushes.setdefault(i, []).append((k, m))
    out = {}
    for i in sorted(pushes):
        try:
            out[i] = stream_live_schedule(plan, pushes[i], max_chunk=max_chunk, input_rate=input_rate)
        except ValueError as e:
            raise ValueError(f"slot {i}: {e}") from None
    return out


class GazeLiveGroup(GazeStreamGroup):
    """A GazeStreamGroup whose slots also answer every pushed frame with its row of a gaze track: GazeStream(live=...) for many
    recordings at once (reach it through GazePredictor.live_group).  live: "hold" or "linear", required; forecast plans only
    (check_live_plan); max_gap defaults to default_max_gap(plan); overlay, alpha and radius as GazeStream takes them.
    Everything a GazeStreamGroup does it does unchanged: the emitted windows are those of a GazeStreamGroup with the same
    arguments on the same ticks, bit for bit.

    The tracks live in one arena, allocated once, when the group is made: sums fp32 (streams, Rt, S/4, S/4) with a count and a
    frame tag per ring slot, Rt = live_ring_slots(plan, max_chunk, max_gap), so the ring of slot i is exactly a GazeStream's
    (ops.group_live_ring).  `capacity` gains "track_slots" and "track_bytes" (per slot), and "total_bytes" includes the arena.

    A round of a tick works in this order, whatever the number of slots:
      1. the samples of all slots (one launch, inputs.group_stft);
      2. their frames (one launch, inputs.group_ingest);
      3. the round's batches (one predict_batch each);
      4. ONE ops.group_live_add: all the windows the round ran, over all slots, in (slot, window) order -- the rows a batch was
         padded with are not among them;
      5. ONE ops.group_live_rows: the frames the round took in, over all slots, in (slot, frame) order; the result is split per
         slot;
      6. ONE ops.group_points_source: the "points_source" and the marker centres of those rows, each under its slot's own params
         row and H x W (infer.points_to_source and marker_centers, bit for bit);
      7. with overlay=True, ONE ops.group_gaze_overlay: the round's chunks of all slots, each of its own size, drawn by one launch
         from a job table (csts_group_gaze_overlay; csts_group_gaze_overlay_yuv when overlay_format names the frames' own
         4:2:0 layout), into views of one allocation.
    That is GazeStream._push's order -- audio, frames, ready windows, fold, rows -- for every slot, so with results_i the windows
    the group emitted for slot i and known_i = group_live_schedule(plan, ticks, max_chunk, input_rate)[i],

      live row of frame f of slot i == row f of fill_track(track_from_windows(results_i[:known_i[f]], f + max_gap + 1), mode=live,
                                                           max_gap=max_gap)

    bit for bit, and the unpredicted row for known 0.  A group of one slot equals a GazeStream with the same batch, live, max_gap
    and overlay on the same pushes: windows, rows and overlay.

    push_live(pieces) -> (windows, live): windows is what push returns, live is {slot: dict} for the slots of pieces, each dict
    exactly a GazeStream.push_live dict ("frame_idx", "known", "points", "peak", "count", "neighbours", "filled", "rescaled",
    "points_source", and "overlay" with overlay=True); the rows of different rounds are concatenated in frame order, and a slot
    that pushed no frames gets the K = 0 dict.  push() folds the windows it runs as well, so push and push_live may be mixed; a
    frame is only answered by the push_live that takes it in.  "points_source" and "overlay" depend on a slot's own H x W; they
    are computed for all slots together (steps 6 and 7) and each slot's are views of the round's: the bytes are those of
    infer.points_to_source and of predictor.render_track on that slot's frames of the round, and a chunk that is not 4-byte
    aligned takes the byte path (packed RGB) or the single-tensor 4:2:0 kernel inside ops.group_gaze_overlay, as render_track
    sends it there.  One case stays per slot: 4:2:0 frames with an RGB overlay (pixel_format "nv12" | "i420" without
    overlay_format) go through predictor.render_track, one inputs.yuv_to_rgb and one csts_gaze_overlay per slot and round,
    because the RGB picture has to be made first; a grouped yuv_to_rgb is a later change.

    close() behaves as in the base class; the closing windows are not folded, as in GazeStream.close (no frame arrives after
    them).  reset(slot) reopens a closed slot and, unlike the base class's, writes to the device: see there.

    Out of scope: live attention maps, different plans per slot, and the command line (tools/predict.py --videos still refuses
    --live and --overlay)."""

    def __init__(self, predictor, streams, live, fps=None, stride=None, segment=None, batch=4, max_chunk=32, pixel_format="rgb24",
                 matrix="bt601", full_range=False, input_rate=None, max_gap=None, overlay=False, alpha=0.4, radius=5,
                 overlay_format=None, window=None):
        from . import ops, inputs
        inputs.no_window(window, "GazeLiveGroup")
        cfg = predictor.cfg                                  # the live arguments are refused before the base class allocates
        self.live, self.overlay, self.alpha, self.radius = live, bool(overlay), float(alpha), int(radius)
        self.max_gap, self.overlay_format, self.track_slots, track_bytes = check_live_args(
            plan_stream(cfg, fps=fps, stride=stride, segment=segment), max_chunk, cfg.DATA.TEST_CROP_SIZE,
            {"pixel_format": pixel_format} if pixel_format in ("nv12", "i420") else {}, live, max_gap, overlay, alpha, radius,
            overlay_format, required=True)
        super().__init__(predictor, streams, fps=fps, stride=stride, segment=segment, batch=batch, max_chunk=max_chunk,
                         pixel_format=pixel_format, matrix=matrix, full_range=full_range, input_rate=input_rate)
        self.capacity = dict(self.capacity, track_slots=self.track_slots, track_bytes=track_bytes,
                             total_bytes=self.capacity["total_bytes"] + self.streams * track_bytes)
        side = self.S // 4
        self._track = ops.group_live_ring(self.streams, self.track_slots, side, side, predictor.device)
        self._answers = None                                 # {slot: [row dicts]} while a push_live runs

    # ---- device work -----------------------------------------------------------------------------------------------------------
    def _round_done(self, ran, chunks):
        """Steps 4 to 7 of a round: fold the windows it ran, answer the frames it took in, then their points_source and overlay."""
        import numpy as np
        import torch
        from . import ops
        took = dict.fromkeys(range(self.streams), 0)
        took.update({i: chunk.shape[0] for i, chunk in chunks})
        if ran:
            dev = ran[0]["heatmaps"].device
            maps = torch.cat([r["heatmaps"] for r in ran], dim=0)
            targets = np.concatenate([np.asarray(r["target_idx"], dtype=np.int64) for r in ran])
            streams = np.concatenate([np.full(len(r["target_idx"]), r["stream"], dtype=np.int32) for r in ran])
            # per slot: the first frame whose row is still to come, minus what a row reads back
            live_from = [max(0, self.frames[i] - took[i] - self.max_gap + 1) for i in range(self.streams)]
            ops.group_live_add(maps, torch.from_numpy(targets).to(dev), torch.from_numpy(streams).to(dev), targets, streams,
                               self._track, live_from)
        if self._answers is None or not chunks:
            return
        first = {i: self.frames[i] - took[i] for i, _ in chunks}
        stream_of = np.concatenate([np.full(took[i], i, dtype=np.int32) for i, _ in chunks])
        frame_of = np.concatenate([np.arange(first[i], first[i] + took[i], dtype=np.int64) for i, _ in chunks])
        rows = ops.group_live_rows(self._track, stream_of, frame_of, mode=self.live, max_gap=self.max_gap,
                                   want=("rescaled", "points", "peak", "count", "neighbours"))
        dev = rows["count"].device
        # what GazeStream._live_rows adds to its rows, for all slots at once; the slots take views of it
        known = np.concatenate([np.full(took[i], self.next_window[i], dtype=np.int32) for i, _ in chunks])
        live_fields(rows, torch.from_numpy(frame_of).to(dev), torch.from_numpy(known).to(dev))
        # step 6: what depends on a slot's own H x W, for all slots at once
        src = ops.group_points_source(rows["points"], [(took[i], self._rows[i], *self.hw[i]) for i, _ in chunks], self.S)
        rows["points_source"] = src["points_source"]
        overlays = None
        if self.overlay and (not self.fmt or self.overlay_format):       # step 7; 4:2:0 in with RGB out stays per slot
            overlays = ops.group_gaze_overlay([(chunk, self._rows[i]) for i, chunk in chunks], rows["rescaled"], src["centers"],
                                              self.S, alpha=self.alpha, radius=self.radius, **self.fmt)
        at = 0
        for n, (i, chunk) in enumerate(chunks):
            self._answers[i].append(self._slot_rows({k: v[at:at + took[i]] for k, v in rows.items()}, chunk,
                                                    None if overlays is None else overlays[n]))
            at += took[i]

    def _slot_rows(self, rows, chunk, overlay):
        """Slot i's rows of one round, sliced from the round's; `overlay` its part of the round's overlay launch, or None when
        there is none: then, with overlay=True, the slot's 4:2:0 frames are drawn in RGB by render_track."""
        if self.overlay:
            rows["overlay"] = overlay if overlay is not None else \
                self.predictor.render_track(chunk, rows, alpha=self.alpha, radius=self.radius, out_format=self.overlay_format,
                                            **self.fmt)
        return rows

    # ---- the interface ---------------------------------------------------------------------------------------------------------
    def push_live(self, pieces):
        """push(pieces) -> (windows, live): windows is what push returns; live is {slot: the GazeStream.push_live dict of the frames
        that slot pushed in this tick, in frame order} for the slots of pieces (K = 0 for a slot without frames).  A tick that is
        refused answers nothing and consumes nothing, as push's."""
        self._answers = {i: [] for i in range(self.streams)}
        try:
            windows = self.push(pieces)
            answers = self._answers
        finally:
            self._answers = None
        side, dev = self.S // 4, self.predictor.device
        return windows, {i: _cat_rows(answers[i]) if answers[i] else live_empty(side, dev, self.hw[i], self.overlay, self.overlay_format)
                         for i in windows}

    def reset(self, slot):
        """Reopen the closed slot `slot` as a fresh stream.  Unlike the base class's, this reset writes to the device: it sets the
        slot's ring to empty (count 0, frame tag -1).  Frame numbers restart at 0 after a reset, so a tag left by the previous
        recording would be taken for a prediction of the new one; the sums need no clearing, a slot restarts when it is retagged."""
        super().reset(slot)
        i = self._slot(slot)
        self._track["count"][i].zero_()
        self._track["frame"][i].fill_(-1)
