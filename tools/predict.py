#!/usr/bin/env python3
"""Gaze predictions of trained weights for one clip or a whole video (one process, one GPU):

    python tools/predict.py --cfg configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml --checkpoint checkpoint_epoch_00015.pyth \
        --clip clip.npz --out gaze.npz [KEY VALUE ...]

--clip: an .npz with frames_u8 uint8 (B, T, H, W, 3), wav fp32 (B, n) at 24 kHz, frames_idx (B, T) and frame_length (scalar), the
arguments of csts_amd.GazePredictor.predict.  Without it a synthetic batch (train.synthetic_batch, --seed) stands in.
--checkpoint: a .pyth file; without it TEST.CHECKPOINT_FILE_PATH of the configuration is used, and with that empty the weights
are the random initialisation.  --out receives points (B, T, 2), peak (B, T), heatmaps and rescaled (B, T, S/4, S/4) as numpy
arrays; one json_stats line reports their shapes and the checkpoint path.

    python tools/predict.py --cfg ... --checkpoint ... --video video.npz [--stride k] [--fps f] --out track.npz

--video: an .npz with frames_u8 uint8 (N, H, W, 3), wav fp32 (n,) at 24 kHz and optionally fps (scalar): the whole recording goes
through csts_amd.GazePredictor.predict_video (windows by csts_amd.plan_video, --stride frames apart) and --out receives the
per-frame track: points (N, 2), peak (N,), count (N,), heatmaps and rescaled (N, S/4, S/4); the json_stats line has
"_type": "predict_video".  --video and --clip exclude each other.
--overlay (with --video): --out also receives points_source (N, 2), the points normalised on the source frame, and overlay uint8
(N, H, W, 3), the track drawn onto the recording (GazePredictor.render_track).  --overlay-dir DIR [--overlay-every K] additionally
writes every K-th overlay frame as DIR/frame_000000.png through PIL; without PIL one line says so and no image is written.
--fill {hold,linear} (with --video): the frames between two neighbouring predictions are filled on the device
(csts_amd.fill_track: the earlier map held, or the time-linear blend of the two), at most --max-gap N frames apart (default:
csts_amd.default_max_gap of the plan).  --out also receives neighbours (N, 2) and filled (N,); the json_stats line gains "fill",
"max_gap" and "filled_frames".  Without --fill the output and the record are what they were.
--attention (one clip or the synthetic batch, not --video): --out also receives the fusion attention maps of
GazePredictor.predict(attention=True): audio_attention, audio_attention_mean, attention_maps, attention_range and
temporal_attention.  --attention-dir DIR (implies --attention; needs --clip, whose uint8 frames are drawn on) additionally writes,
as the reference's vis_av_st_fusion does, DIR/spat_attn_<clip>_<frame>_head_<k>.png for every head and ..._head_mean.png
(GazePredictor.render_attention, through PIL; without PIL one line says so and no image is written) and
DIR/temporal_attn_<clip>.txt.  These per-clip arrays are not defined yet for a whole recording: --attention with --video is an
error; a recording has --attention-track.
--attention-track (with --video): the fusion attention over the whole recording (GazePredictor.predict_video(attention_track=True),
csts_attention_track): --out also receives attention_maps and attention_mixed (N, heads + 1, h, w), attention_range
(N, heads + 1, 2), attention_count (N,) and temporal_attention_windows (windows, n, n); with --fill the attention track is filled
too and attention_neighbours (N, 2) and attention_filled (N,) are added.  The json_stats line gains "attention_track" and
"attention_frames" (frames a map was computed for).  --attention-overlay HEAD|mean (implies --attention-track): --out also
receives attention_overlay uint8 (N, H, W, 3), that head's map (or the head mean) drawn onto the recording with the gaze track's
points as discs (GazePredictor.render_attention_track).  Without these flags the output and the record are what they were.
Audio at another rate (--clip and --video): an optional npz entry sample_rate (integer scalar) says what rate wav was recorded at,
--sample-rate R overrides it; wav, floating or int16, may then carry a channel axis in front of its samples ((B, C, n) / (C, n)),
and is brought to 24 kHz mono on the device first (csts_amd.inputs.resample_audio).  --out then also records sample_rate (what
came in) and audio_rate (24000), and the json_stats line carries both.  Without either the output and the record are what they
were.
4:2:0 pictures (--clip and --video): instead of frames_u8 the npz may hold frames_yuv uint8 (B, T, H * 3 / 2, W) / (N, H * 3 / 2, W)
with a pixel_format entry ("nv12" or "i420") and optionally yuv_matrix ("bt601", the default, or "bt709") and yuv_full_range;
--pixel-format, --yuv-matrix and --yuv-full-range override the entries.  The pictures are uploaded and sampled in that format
(half the bytes of RGB); overlays are RGB uint8 (N, H, W, 3) unless --overlay-format nv12 | i420 names the recording's own layout:
overlay / live_overlay are then drawn in that format, uint8 (N, H * 3 / 2, W) (GazePredictor.render_track(out_format=...)), --out
gains the entry overlay_pixel_format, and --overlay-dir writes its PNGs from inputs.yuv_to_rgb_host of them.  An npz holding both
frames_u8 and frames_yuv is an error.  The json_stats line then carries "pixel_format".
Decoder surfaces: frames_yuv may hold padded surfaces (..., Hs * 3 / 2, Ws) -- a row pitch and a coded height larger than the
picture -- with the entry yuv_window int (4,) = (top, left, H, W), the picture inside them (csts_amd.inputs.check_window);
--yuv-window TOP LEFT H W overrides the entry.  Both need frames_yuv.  The surfaces are uploaded as they are and read in place; the
result is that of the repacked pictures (inputs.yuv_window).  --out and the json_stats line carry yuv_window; an RGB overlay and
the --overlay-dir PNGs show the window, a 4:2:0 overlay has the surfaces' shape.  --videos takes tight pictures only.
--stream [--chunk K] (with --video): the recording is replayed through csts_amd.GazeStream (GazePredictor.stream) in pushes of K
frames (default 8) with the matching audio -- the samples up to frame_end * 24000 / fps, the rest with the last push -- as a live
source would deliver it, and closed.  --out receives the same entries as --video, the track folded from the emitted windows by
csts_amd.track_from_windows, plus stream_windows (the window numbers, in the order they were emitted) and stream_dropped; the
json_stats line gains "stream", "chunk" and "dropped".  A recording at another rate (sample_rate entry or --sample-rate) is pushed
at that rate, int16 and (C, n) as stored -- the samples up to frame_end * rate / fps -- and resampled inside the stream with the
filter state carried from push to push (GazePredictor.stream(input_rate=rate)); --out records sample_rate and audio_rate as the
offline path does.  --fps must then be integral (a stream places its audio by the exact ratio of columns to frames); --overlay
(without --live), --fill and --attention are not part of the stream.
--stream --attention-track: the stream runs with attention=True and --out also receives the attention track entries of
--attention-track, folded from the emitted windows by csts_amd.attention_track_from_windows.  With --live it also receives
live_attention_frame (N,) int64 (the frame whose map a row holds, -1: none), live_attention_count (N,), live_attention_maps
(N, heads + 1, h, w) and live_attention_range (N, heads + 1, 2): the newest map at most default_attention_age(plan) frames old
(GazeStream states the rule), and with --overlay --attention-overlay HEAD|mean live_attention_overlay, the frames with that map
drawn over as they arrived.  What the stream refuses (--attention-overlay without --live and --overlay) is refused with its
message.
--videos A.npz B.npz ... --stream [--chunk K] [--batch B]: the recordings are replayed as the slots of ONE csts_amd.GazeStreamGroup
(GazePredictor.stream_group(len(videos), batch=B)): every tick pushes the next K frames of every recording that still has some,
with the samples that belong to them, cut exactly as --video --stream cuts one recording; a recording that ends is closed.  The
windows of different recordings that become ready in the same tick are predicted together, B per forward.  The recordings share
one plan: the same fps, sample rate and pixel format.  --out OUT names one file per recording, OUT with _<slot> before its
extension, each with the entries --video --stream writes plus stream_slot and stream_batches int64 (batches, B, 2): the (slot,
window) rows of every batch this slot took part in, rows a short batch lacks as (-1, -1); one json_stats line per recording.
--videos without --stream, or with --live, --overlay or the attention flags, is refused.
--live {hold,linear} (with --stream, forecast configurations): every pushed frame is answered with its row of the live gaze track
(GazeStream.push_live: the forecast shown on the frame it was made for, when that frame arrives, from the windows that had run by
then; the frames between two predictions at most --max-gap apart, default csts_amd.default_max_gap of the plan, hold the earlier
map or blend the two).  --out also receives live_points (N, 2), live_peak, live_count, live_known (the windows each row was
computed from), live_filled and live_points_source (N, 2), and with --overlay live_overlay uint8 (N, H, W, 3), the frames drawn over
as they arrived; --overlay-dir writes those frames as PNGs.  The entries written without --live stay as they are; the json_stats
line gains "live", "max_gap" and "live_filled_frames".  --fill stays an offline flag: the mode of a live track is --live's."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd.config import assert_and_infer_cfg, load_yaml      # noqa: E402
from csts_amd.infer import GazePredictor                         # noqa: E402
from csts_amd import inputs                                      # noqa: E402
from csts_amd.inputs import AUDIO_RATE                           # noqa: E402

CLIP_KEYS = ("frames_u8", "wav", "frames_idx", "frame_length")
VIDEO_KEYS = ("frames_u8", "wav")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="CSTS (MI355X) gaze prediction.")
    p.add_argument("--cfg", dest="cfg_file", default=os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"), type=str)
    p.add_argument("--checkpoint", default=None, type=str, help=".pyth file (default: TEST.CHECKPOINT_FILE_PATH)")
    p.add_argument("--clip", default=None, type=str, help=".npz with " + ", ".join(CLIP_KEYS))
    p.add_argument("--video", default=None, type=str, help=".npz with " + ", ".join(VIDEO_KEYS) + " [, fps]: a whole recording")
    p.add_argument("--videos", default=None, nargs="+", type=str, metavar="NPZ",
                   help="with --stream: several recordings replayed as the slots of one stream group (--batch windows per forward)")
    p.add_argument("--stride", default=None, type=int, help="frames between windows of --video (default: csts_amd.plan_video's)")
    p.add_argument("--fps", default=None, type=float, help="frame rate of --video (default: its fps entry, else DATA.TARGET_FPS)")
    p.add_argument("--overlay", action="store_true", help="with --video: add points_source and the rendered overlay to --out")
    p.add_argument("--overlay-dir", default=None, type=str, help="with --video: also write overlay frames as PNGs here (implies --overlay)")
    p.add_argument("--overlay-every", default=1, type=int, help="write every K-th frame to --overlay-dir")
    p.add_argument("--overlay-format", default=None, choices=("rgb24", "nv12", "i420"),
                   help="with --overlay on a 4:2:0 recording: draw the overlay in the recording's own layout instead of RGB")
    p.add_argument("--fill", default=None, choices=["hold", "linear"], help="with --video: fill the frames between predictions")
    p.add_argument("--max-gap", default=None, type=int, help="with --fill: widest distance between two predictions that is filled")
    p.add_argument("--attention", action="store_true", help="add the fusion attention maps to --out (one clip, not --video)")
    p.add_argument("--attention-dir", default=None, type=str,
                   help="with --clip: also write the attention overlays as PNGs and the temporal matrices as text here (implies --attention)")
    p.add_argument("--attention-track", action="store_true", help="with --video: add the whole-recording attention track to --out")
    p.add_argument("--attention-overlay", default=None, type=str, metavar="HEAD|mean",
                   help="with --video: also draw that head's attention track onto the recording (implies --attention-track)")
    p.add_argument("--sample-rate", default=None, type=int,
                   help="rate wav was recorded at (default: the npz entry sample_rate, else 24000): resampled on the device")
    p.add_argument("--pixel-format", default=None, choices=["nv12", "i420"],
                   help="layout of the npz entry frames_yuv (default: its pixel_format entry)")
    p.add_argument("--yuv-matrix", default=None, choices=["bt601", "bt709"],
                   help="colour matrix of frames_yuv (default: the npz entry yuv_matrix, else bt601)")
    p.add_argument("--yuv-full-range", default=None, type=int, choices=[0, 1],
                   help="1: frames_yuv is full range, 0: limited (default: the npz entry yuv_full_range, else limited)")
    p.add_argument("--yuv-window", default=None, nargs=4, type=int, metavar=("TOP", "LEFT", "H", "W"),
                   help="the picture inside the padded surfaces of frames_yuv (default: the npz entry yuv_window, else the whole)")
    p.add_argument("--stream", action="store_true", help="with --video: replay the recording through GazePredictor.stream")
    p.add_argument("--chunk", default=None, type=int, help="with --stream: frames per push (default 8)")
    p.add_argument("--live", default=None, choices=["hold", "linear"],
                   help="with --stream: answer every pushed frame with its row of the live gaze track (honours --max-gap, --overlay)")
    p.add_argument("--seed", default=2000, type=int, help="seed of the synthetic batch used without --clip")
    p.add_argument("--batch", default=2, type=int,
                   help="clips in the synthetic batch used without --clip; with --videos: windows per forward of the stream group")
    p.add_argument("--no-graph", action="store_true", help="launch the kernels eagerly instead of replaying a HIP graph")
    p.add_argument("--out", required=True, type=str, help=".npz to write")
    p.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="KEY VALUE overrides")
    args = p.parse_args(argv)
    if args.video is not None and args.clip is not None:
        p.error("--video and --clip exclude each other: a whole recording or one clip")
    if args.videos is not None:
        if args.video is not None or args.clip is not None:
            p.error("--videos, --video and --clip exclude each other: several recordings, a whole recording or one clip")
        if not args.stream:
            p.error("--videos replays several recordings as the slots of one stream group: it needs --stream (predict one "
                    "recording offline with --video)")
        if args.live is not None or args.overlay or args.overlay_dir or args.attention or args.attention_dir or \
                args.attention_track or args.attention_overlay is not None or args.fill is not None:
            p.error("--videos serves the windows of several recordings together: --live, --overlay, --fill and the attention flags "
                    "are not part of a stream group (use --video --stream for one recording)")
        if args.batch < 1:
            p.error("--batch must be positive")
    if (args.overlay or args.overlay_dir) and args.video is None:
        p.error("--overlay and --overlay-dir draw onto a recording: they need --video")
    if (args.attention or args.attention_dir) and args.video is not None:
        p.error("--attention and --attention-dir show one clip's fusion attention: they do not work with --video (the per-clip "
                "arrays are not defined yet for a whole recording); use --clip, or --attention-track for the recording's track")
    if (args.attention_track or args.attention_overlay is not None) and args.video is None:
        p.error("--attention-track and --attention-overlay follow the attention over a recording: they need --video")
    if args.attention_overlay is not None and args.attention_overlay != "mean":
        try:
            if int(args.attention_overlay) < 0:
                raise ValueError
        except ValueError:
            p.error("--attention-overlay takes a head index (0, 1, ...) or mean")
    if args.attention_dir is not None and args.clip is None:
        p.error("--attention-dir draws onto a clip's uint8 frames: it needs --clip")
    if args.fill is not None and args.video is None:
        p.error("--fill fills the track of a recording: it needs --video")
    if args.max_gap is not None and args.fill is None and args.live is None:
        p.error("--max-gap belongs to a fill mode: it needs --fill")
    if args.max_gap is not None and args.max_gap < 1:
        p.error("--max-gap must be positive")
    if args.overlay_every < 1:
        p.error("--overlay-every must be positive")
    if args.overlay_format is not None and not (args.overlay or args.overlay_dir):
        p.error("--overlay-format names the format of the overlay: it needs --overlay or --overlay-dir")
    if args.stream and args.video is None and args.videos is None:
        p.error("--stream replays a recording as a live stream: it needs --video")
    if args.chunk is not None and not args.stream:
        p.error("--chunk is the push size of --stream")
    if args.chunk is not None and args.chunk < 1:
        p.error("--chunk must be positive")
    if args.live is not None and not args.stream:
        p.error("--live answers the frames of a replayed stream: it needs --stream")
    if args.stream and (args.fill or ((args.overlay or args.overlay_dir) and args.live is None)):
        p.error("--stream emits windows as they complete: --overlay and --fill are not part of it (fold the "
                "windows with csts_amd.track_from_windows, then fill_track / render_track; --live hold|linear draws the live "
                "track, with --overlay onto the frames as they arrive)")
    if args.sample_rate is not None and args.sample_rate < 1:
        p.error("--sample-rate must be positive")
    if (args.pixel_format or args.yuv_matrix or args.yuv_full_range is not None or args.yuv_window is not None) \
            and args.video is None and args.clip is None and args.videos is None:
        p.error("--pixel-format, --yuv-matrix, --yuv-full-range and --yuv-window describe recorded pictures: they need --clip or "
                "--video")
    if args.sample_rate is not None and args.video is None and args.clip is None and args.videos is None:
        p.error("--sample-rate is the rate of a recorded waveform: it needs --clip or --video")
    return args


def source_rate(z, args, path):
    """The rate the waveform of an opened npz was recorded at: --sample-rate, else its sample_rate entry, else None (24 kHz)."""
    if args.sample_rate is not None:
        return int(args.sample_rate)
    if "sample_rate" not in z.files:
        return None
    rate = np.asarray(z["sample_rate"]).reshape(-1)
    if rate.size != 1 or float(rate[0]) != int(rate[0]) or int(rate[0]) < 1:
        raise SystemExit(f"{path}: sample_rate must be one positive integer, got {z['sample_rate']!r}")
    return int(rate[0])


def pictures(z, args, path, lead):
    """The pictures of an opened npz (numpy) and the keywords that name their format ({} for frames_u8, packed RGB): frames_yuv
    with pixel_format [, yuv_matrix, yuv_full_range, yuv_window], each overridden by its flag.  lead: 1 for a video (N, ...), 2 for
    a clip."""
    from csts_amd.datasets import clip_pictures
    if "frames_yuv" not in z.files and (args.pixel_format or args.yuv_matrix or args.yuv_full_range is not None):
        raise SystemExit(f"{path} holds no frames_yuv: --pixel-format, --yuv-matrix and --yuv-full-range describe 4:2:0 pictures")
    if "frames_yuv" not in z.files and (args.yuv_window is not None or "yuv_window" in z.files):
        raise SystemExit(f"{path} holds no frames_yuv: --yuv-window and the entry yuv_window name the picture inside 4:2:0 surfaces")
    try:
        frames, _, _, fmt = clip_pictures(z, path, args.pixel_format, args.yuv_matrix,
                                          None if args.yuv_full_range is None else bool(args.yuv_full_range), lead=lead)
    except ValueError as e:
        raise SystemExit(str(e))
    kw = {} if fmt[0] == "rgb24" else {"pixel_format": fmt[0], "matrix": fmt[1], "full_range": fmt[2]}
    window = args.yuv_window if args.yuv_window is not None else (z["yuv_window"] if "yuv_window" in z.files else None)
    if window is not None:
        window = np.asarray(window).reshape(-1).tolist()
        try:
            kw["window"] = inputs.check_window(frames.shape, fmt[0], window)
        except ValueError as e:
            raise SystemExit(f"{path}: {e}")
    return frames, kw


def waveform(z, rate, dev):
    """wav of an opened npz on the device: fp32 as before without a rate; with one, int16 stays int16 (the kernel scales it)."""
    wav = torch.from_numpy(z["wav"])
    return (wav if rate is not None and wav.dtype == torch.int16 else wav.float()).to(dev)


def replay_stream(predictor, frames, wav, fps, stride, chunk, fmt, rate=None, live=None, max_gap=None, overlay=False,
                  overlay_format=None, attention=False, attention_overlay=None):
    """The recording pushed through GazePredictor.stream in pushes of `chunk` frames with the matching audio, then closed ->
    (the track by track_from_windows with "windows" = their number, the window numbers in emission order, the dropped count).
    rate: the rate wav, (n,) or (C, n), was recorded at; the stream resamples it (input_rate).  live "hold" | "linear": the pushes
    go through push_live and the track gains "live" = the rows of all N frames (GazeStream.push_live's dict) and "live_max_gap".
    attention: the stream runs with attention=True and the track gains attention_track_from_windows' entries; attention_overlay
    ("mean" or a head index) is the stream's."""
    from fractions import Fraction
    from csts_amd import attention_track_from_windows, track_from_windows
    more = {"attention": True, "attention_overlay": attention_overlay} if attention else {}
    stream = predictor.stream(fps=fps, stride=stride, input_rate=rate, live=live, max_gap=max_gap, overlay=overlay,
                              overlay_format=overlay_format, **more, **fmt)
    N, n = frames.shape[0], wav.shape[-1]
    per = Fraction(AUDIO_RATE if rate is None else rate) / stream.plan["fps"]     # samples per frame
    results, rows, sent = [], [], 0
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        upto = n if b == N else min(n, int(b * per))
        piece = wav[..., sent:upto] if upto > sent else None
        if live is None:
            results += stream.push(frames[a:b], piece)
        else:
            done, answered = stream.push_live(frames[a:b], piece)
            results += done
            rows.append(answered)
        sent = max(sent, upto)
    results += stream.close()
    if not results:
        raise SystemExit(f"the stream of {N} frames and {n} samples completed no window (one window observes "
                         f"{stream.plan['observed']} frames)")
    track = track_from_windows(results, N)
    if attention:
        track.update(attention_track_from_windows(results, N, stream.S))
    if live is not None:
        track["live"] = {k: torch.cat([r[k] for r in rows], dim=0) for k in rows[0]}
        track["live_max_gap"] = stream.max_gap
    return track, [r["window"] for r in results], stream.dropped


def replay_group(predictor, recordings, fps, stride, chunk, batch, fmt, rate=None):
    """The recordings [(frames, wav)] replayed as the slots of one GazePredictor.stream_group: every tick pushes the next `chunk`
    frames of every recording that still has some with the matching audio (replay_stream's cut), and a recording that ends is
    closed -> per slot (the track by track_from_windows, the window numbers in emission order, the dropped count, the batches the
    slot took part in as lists of (slot, window) rows)."""
    from fractions import Fraction
    from csts_amd import track_from_windows
    group = predictor.stream_group(len(recordings), fps=fps, stride=stride, batch=batch, input_rate=rate, **fmt)
    per = Fraction(AUDIO_RATE if rate is None else rate) / group.plan["fps"]      # samples per frame
    results, sent, batches = [[] for _ in recordings], [0] * len(recordings), []
    for a in range(0, max(frames.shape[0] for frames, _ in recordings), chunk):
        pieces, ending = {}, []
        for i, (frames, wav) in enumerate(recordings):
            N, n = frames.shape[0], wav.shape[-1]
            if a >= N:
                continue
            b = min(a + chunk, N)
            upto = n if b == N else min(n, int(b * per))
            pieces[i] = (frames[a:b], wav[..., sent[i]:upto] if upto > sent[i] else None)
            sent[i] = max(sent[i], upto)
            if b == N:
                ending.append(i)
        done = [group.push(pieces)]
        batches += group.batches
        for i in ending:
            done.append(group.close(i))
            batches += group.batches
        for res in done:
            for i, rs in res.items():
                results[i] += rs
    out = []
    for i, (frames, wav) in enumerate(recordings):
        if not results[i]:
            raise SystemExit(f"recording {i} of {frames.shape[0]} frames and {wav.shape[-1]} samples completed no window (one "
                             f"window observes {group.plan['observed']} frames)")
        out.append((track_from_windows(results[i], frames.shape[0]), [r["window"] for r in results[i]], group.dropped[i],
                    [rows for rows in batches if any(slot == i for slot, _ in rows)]))
    return out


def predict_group(args, predictor, dev):
    """--videos: load the recordings, replay them through one stream group, write one file per recording."""
    recordings, shared = [], None
    for path in args.videos:
        if not os.path.exists(path):
            raise SystemExit(f"{path}: no such file")
        with np.load(path) as z:
            missing = [k for k in VIDEO_KEYS if k not in z.files and (k != "frames_u8" or "frames_yuv" not in z.files)]
            if missing:
                raise SystemExit(f"{path} lacks {missing}: a video holds {list(VIDEO_KEYS)} and optionally fps")
            pics, fmt = pictures(z, args, path, lead=1)
            fps = args.fps if args.fps is not None else (float(z["fps"]) if "fps" in z.files else None)
            rate = source_rate(z, args, path)
            if shared is None:
                shared = (fps, rate, fmt)
            elif shared != (fps, rate, fmt):
                raise SystemExit(f"{path}: the slots of a stream group share one plan: fps, sample rate and pixel format "
                                 f"{(fps, rate, fmt)} differ from {args.videos[0]}'s {shared}")
            recordings.append((torch.from_numpy(pics).to(dev), waveform(z, rate, dev)))
    fps, rate, fmt = shared
    if "window" in fmt:
        raise SystemExit("--videos serves tight 4:2:0 pictures only: yuv_window / --yuv-window belong to --video and --clip")
    chunk = 8 if args.chunk is None else args.chunk
    try:
        done = replay_group(predictor, recordings, fps, args.stride, chunk, args.batch, fmt, rate)
    except ValueError as e:
        raise SystemExit(str(e))
    stem, ext = os.path.splitext(args.out)
    rates = {} if rate is None else {"sample_rate": np.int64(rate), "audio_rate": np.int64(AUDIO_RATE)}
    for i, (track, windows, dropped, batches) in enumerate(done):
        arrays = {k: track[k].cpu().numpy() for k in ("points", "peak", "count", "rescaled", "heatmaps")}
        rows = np.full((len(batches), args.batch, 2), -1, dtype=np.int64)
        for j, batch in enumerate(batches):
            rows[j, :len(batch)] = batch
        arrays.update(stream_windows=np.asarray(windows, dtype=np.int64), stream_dropped=np.int64(dropped), stream_slot=np.int64(i),
                      stream_batches=rows)
        out = f"{stem}_{i}{ext}"
        np.savez(out, **arrays, **rates)
        record = {"_type": "predict_video", "checkpoint": predictor.checkpoint_path, "source": args.videos[i],
                  "graph": predictor.graph, "out": out, "windows": track["windows"], "frames": int(arrays["count"].shape[0]),
                  "covered_frames": int((arrays["count"] > 0).sum()), "shapes": {k: list(v.shape) for k, v in arrays.items()},
                  "stream": True, "chunk": chunk, "dropped": int(dropped), "stream_slot": i, "streams": len(done),
                  "batch": args.batch, "batches": len(batches)}
        record.update({k: int(v) for k, v in rates.items()})
        if fmt:
            record["pixel_format"] = fmt["pixel_format"]
        print("json_stats: " + json.dumps(record), flush=True)


def write_pngs(overlay, directory, every, fmt=None):
    """Every `every`-th overlay frame as a PNG.  fmt: the format keywords of a 4:2:0 overlay (N, H * 3 / 2, W), whose frames are
    converted by the library's own rule on the host (inputs.yuv_to_rgb_host); None for RGB (N, H, W, 3)."""
    try:
        from PIL import Image
    except ImportError:
        print(f"PIL is not installed: no PNG written to {directory}", flush=True)
        return
    os.makedirs(directory, exist_ok=True)
    for i in range(0, overlay.shape[0], every):
        picture = overlay[i] if fmt is None else inputs.yuv_to_rgb_host(overlay[i], **fmt)
        Image.fromarray(picture).save(os.path.join(directory, f"frame_{i:06d}.png"))


def write_attention(predictor, frames_u8, out, directory, fmt):
    """spat_attn_<clip>_<frame>_head_<k>.png for every head and the head mean, temporal_attn_<clip>.txt."""
    os.makedirs(directory, exist_ok=True)
    temporal = out["temporal_attention"].cpu().numpy()
    for b in range(temporal.shape[0]):
        np.savetxt(os.path.join(directory, f"temporal_attn_{b}.txt"), temporal[b])
    try:
        from PIL import Image
    except ImportError:
        print(f"PIL is not installed: no PNG written to {directory}", flush=True)
        return
    heads = out["attention_maps"].shape[1] - 1
    for k in list(range(heads)) + [None]:
        drawn = predictor.render_attention(frames_u8, out, head=k, **fmt).cpu().numpy()
        name = "mean" if k is None else str(k)
        for b in range(drawn.shape[0]):
            for t in range(drawn.shape[1]):
                Image.fromarray(drawn[b, t]).save(os.path.join(directory, f"spat_attn_{b}_{t}_head_{name}.png"))


def main(argv=None):
    args = parse_args(argv)
    attention = bool(args.attention or args.attention_dir)
    npz, pics = args.video or args.clip, None
    if npz is not None and os.path.exists(npz):  # the pictures are read, and a bad npz refused, before the model is built
        with np.load(npz) as z:
            if "frames_u8" in z.files or "frames_yuv" in z.files:
                pics = pictures(z, args, npz, lead=1 if args.video is not None else 2)
    overlay_yuv = args.overlay_format in ("nv12", "i420")
    if overlay_yuv and pics is not None and pics[1].get("pixel_format") != args.overlay_format:
        raise SystemExit(f"--overlay-format {args.overlay_format} draws the overlay in the recording's own layout, and "
                         f"{npz} holds {pics[1].get('pixel_format', 'rgb24')} frames")
    cfg = assert_and_infer_cfg(load_yaml(args.cfg_file, ["NUM_GPUS", 1] + list(args.opts or [])))
    if not torch.cuda.is_available():
        raise SystemExit("tools/predict.py needs an MI355X: there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(cfg.RNG_SEED)
    predictor = GazePredictor(cfg, args.checkpoint, device=dev, graph=not args.no_graph)
    if args.videos is not None:
        predict_group(args, predictor, dev)
        return
    if args.video is not None:
        attention_track = bool(args.attention_track or args.attention_overlay is not None)
        with np.load(args.video) as z:
            missing = [k for k in VIDEO_KEYS if k not in z.files and (k != "frames_u8" or "frames_yuv" not in z.files)]
            if missing:
                raise SystemExit(f"{args.video} lacks {missing}: a video holds {list(VIDEO_KEYS)} and optionally fps")
            fps = args.fps if args.fps is not None else (float(z["fps"]) if "fps" in z.files else None)
            rate = source_rate(z, args, args.video)
            frames, fmt = torch.from_numpy(pics[0]).to(dev), pics[1]
            if args.stream:
                try:
                    out, stream_windows, dropped = replay_stream(predictor, frames, waveform(z, rate, dev), fps, args.stride,
                                                                 8 if args.chunk is None else args.chunk, fmt, rate, live=args.live,
                                                                 max_gap=args.max_gap, overlay=bool(args.overlay or args.overlay_dir),
                                                                 overlay_format=args.overlay_format, attention=attention_track,
                                                                 attention_overlay=args.attention_overlay
                                                                 if args.attention_overlay in (None, "mean")
                                                                 else int(args.attention_overlay))
                except ValueError as e:
                    raise SystemExit(str(e))
            else:
                out = predictor.predict_video(frames, waveform(z, rate, dev), sample_rate=rate,
                                              fps=fps, stride=args.stride, overlay=bool(args.overlay or args.overlay_dir),
                                              fill=args.fill, max_gap=args.max_gap, attention_track=attention_track,
                                              overlay_format=args.overlay_format, **fmt)
            if args.attention_overlay is not None and not args.stream:
                head = None if args.attention_overlay == "mean" else int(args.attention_overlay)
                out["attention_overlay"] = predictor.render_attention_track(frames, out, head=head, points=out["points"], **fmt)
        keys = ("points", "peak", "count", "rescaled", "heatmaps") + (("points_source", "overlay") if "overlay" in out else ())
        keys += ("neighbours", "filled") if args.fill is not None else ()
        if attention_track:
            keys += ("attention_maps", "attention_range", "attention_mixed", "attention_count", "temporal_attention_windows")
            keys += ("attention_neighbours", "attention_filled") if args.fill is not None else ()
            keys += ("attention_overlay",) if args.attention_overlay is not None and not args.stream else ()
        arrays = {k: out[k].cpu().numpy() for k in keys}
        rates = {} if rate is None else {"sample_rate": np.int64(rate), "audio_rate": np.int64(AUDIO_RATE)}
        if args.stream:
            arrays["stream_windows"] = np.asarray(stream_windows, dtype=np.int64)
            arrays["stream_dropped"] = np.int64(dropped)
        if args.live is not None:
            live_keys = ("points", "peak", "count", "known", "filled", "points_source") + (("overlay",) if "overlay" in out["live"] else ())
            if attention_track:
                live_keys += ("attention_frame", "attention_count", "attention_maps", "attention_range")
                live_keys += ("attention_overlay",) if "attention_overlay" in out["live"] else ()
            arrays.update({"live_" + k: out["live"][k].cpu().numpy() for k in live_keys})
        if args.overlay_format is not None:
            arrays["overlay_pixel_format"] = np.array(args.overlay_format)
        if "window" in fmt:
            arrays["yuv_window"] = np.asarray(fmt["window"], dtype=np.int64)
        np.savez(args.out, **arrays, **rates)
        if args.overlay_dir is not None:
            write_pngs(arrays["live_overlay" if args.live is not None else "overlay"], args.overlay_dir, args.overlay_every,
                       fmt if overlay_yuv else None)
        record = {"_type": "predict_video", "checkpoint": predictor.checkpoint_path, "source": args.video,
                  "graph": predictor.graph, "out": args.out, "windows": out["windows"],
                  "frames": int(arrays["count"].shape[0]),
                  "covered_frames": int((arrays["count"] > 0).sum()),
                  "shapes": {k: list(v.shape) for k, v in arrays.items()}}
        record.update({k: int(v) for k, v in rates.items()})
        if fmt:
            record["pixel_format"] = fmt["pixel_format"]
        if "window" in fmt:
            record["yuv_window"] = list(fmt["window"])
        if args.fill is not None:
            record.update({"fill": args.fill, "max_gap": int(out["max_gap"]), "filled_frames": int(arrays["filled"].sum())})
        if args.stream:
            record.update({"stream": True, "chunk": 8 if args.chunk is None else args.chunk, "dropped": int(dropped)})
        if args.live is not None:
            record.update({"live": args.live, "max_gap": int(out["live_max_gap"]), "live_filled_frames": int(arrays["live_filled"].sum())})
        if attention_track:
            frames = arrays["attention_count"] > 0
            if args.fill is not None:
                frames = frames | arrays["attention_filled"]
            record.update({"attention_track": True, "attention_frames": int(frames.sum())})
        print("json_stats: " + json.dumps(record), flush=True)
        return
    if args.clip is not None:
        with np.load(args.clip) as z:
            missing = [k for k in CLIP_KEYS if k not in z.files and (k != "frames_u8" or "frames_yuv" not in z.files)]
            if missing:
                raise SystemExit(f"{args.clip} lacks {missing}: a clip holds {list(CLIP_KEYS)}")
            frames_u8, fmt = torch.from_numpy(pics[0]).to(dev), pics[1]
            rate = source_rate(z, args, args.clip)
            out = predictor.predict(frames_u8, waveform(z, rate, dev), torch.from_numpy(z["frames_idx"]).float().to(dev),
                                    float(z["frame_length"]), attention=attention, sample_rate=rate, **fmt)
        if args.attention_dir is not None:
            write_attention(predictor, frames_u8, out, args.attention_dir, fmt)
        source = args.clip
    else:
        from csts_amd import train as T
        batch = T.synthetic_batch(args.batch, cfg.DATA.NUM_FRAMES, cfg.DATA.TEST_CROP_SIZE, args.seed, dev,
                                  spatial=T.spatial_config(cfg, train=False))
        out = predictor.predict_batch(batch, attention=attention)
        source = f"synthetic_batch(seed={args.seed})"
        rate, fmt = None, {}
    keys = ("points", "peak", "rescaled", "heatmaps")
    if attention:
        keys += ("audio_attention", "audio_attention_mean", "attention_maps", "attention_range", "temporal_attention")
    arrays = {k: out[k].cpu().numpy() for k in keys}
    rates = {} if rate is None else {"sample_rate": np.int64(rate), "audio_rate": np.int64(AUDIO_RATE)}
    if "window" in fmt:
        arrays["yuv_window"] = np.asarray(fmt["window"], dtype=np.int64)
    np.savez(args.out, **arrays, **rates)
    record = {"_type": "predict", "checkpoint": predictor.checkpoint_path, "source": source, "graph": predictor.graph,
              "out": args.out, "shapes": {k: list(v.shape) for k, v in arrays.items()}}
    record.update({k: int(v) for k, v in rates.items()})
    if fmt:
        record["pixel_format"] = fmt["pixel_format"]
    if "window" in fmt:
        record["yuv_window"] = list(fmt["window"])
    print("json_stats: " + json.dumps(record), flush=True)


if __name__ == "__main__":
    main()
