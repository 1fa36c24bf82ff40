#!/usr/bin/env python3
"""Write a small random data set in the layout csts_amd/datasets.py reads (CSTS_AMD.DATA_ROOT), to try the recorded-clip path:

    python tools/make_toy_dataset.py --out /tmp/toy
    python tools/run_net.py --cfg configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml CSTS_AMD.SYNTHETIC_DATA False \
        CSTS_AMD.DATA_ROOT /tmp/toy TRAIN.BATCH_SIZE 2 TEST.BATCH_SIZE 2 SOLVER.MAX_EPOCH 1 LOG_PERIOD 1

  train.csv, test.csv                         <video>/<video>_t<start>_t<end>.mp4, one clip per line
  clips/<video>/<clip>.npz                    frames_u8 uint8 (N, H, W, 3) noise, wav fp32 (n,) noise at 24 kHz, fps
  gaze_frame_label/<video>_frame_label.csv    header, then one row per video frame: frame, x, y, type (Ego4D) or
                                              frame, time, x, y, type (Aria)

--dataset picks the clip length (Ego4D forecast: 150 frames of 5 s; Aria forecast: 100 frames of 5 s at 20 fps).  train.csv lists
every clip, test.csv the last --test-clips of them.  --sample-rate R writes the waveforms at R Hz instead, with a sample_rate entry
beside them (csts_amd/datasets.py resamples such clips to 24 kHz on the device).  --pixel-format nv12|i420 writes the pictures as
random 4:2:0 frames instead: frames_yuv uint8 (N, H * 3 / 2, W) with a pixel_format entry (H and W must be even).  Pure numpy: no
GPU needed."""
import argparse
import os

import numpy as np

CLIP = {"ego4d_av_gaze_forecast": (150, 30, ("frame", "x", "y", "type")),
        "aria_av_gaze_forecast": (100, 20, ("frame", "time", "x", "y", "type"))}


def write_dataset(out, dataset="ego4d_av_gaze_forecast", clips_per_video=(3, 2), sizes=((36, 48), (40, 44)), seconds=5,
                  test_clips=2, seed=0, label_rows=None, sample_rate=None, pixel_format="rgb24"):
    """-> the list of clip lines written to train.csv.  clips_per_video[v] clips of sizes[v % len(sizes)] = (H, W) for video v;
    label_rows (optional): rows of every video's label table (default: enough for every clip), to make a table run out.
    sample_rate (optional): the waveforms are noise at that rate and every clip carries a sample_rate entry.
    pixel_format "nv12" | "i420": every clip holds frames_yuv uint8 (N, H * 3 / 2, W) noise and a pixel_format entry."""
    if pixel_format not in ("rgb24", "nv12", "i420"):
        raise ValueError(f"pixel_format must be rgb24, nv12 or i420, got {pixel_format!r}")
    n_frames, fps, header = CLIP[dataset]
    rng = np.random.default_rng(seed)
    lines = []
    os.makedirs(os.path.join(out, "gaze_frame_label"), exist_ok=True)
    for v, nclips in enumerate(clips_per_video):
        video = f"video{v:02d}"
        H, W = sizes[v % len(sizes)]
        os.makedirs(os.path.join(out, "clips", video), exist_ok=True)
        for c in range(nclips):
            name = f"{video}_t{c * seconds}_t{(c + 1) * seconds}"
            rate = {} if sample_rate is None else {"sample_rate": np.int64(sample_rate)}
            if pixel_format == "rgb24":
                pictures = {"frames_u8": rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8)}
            else:
                if H % 2 or W % 2:
                    raise ValueError(f"4:2:0 frames need even H and W, got {H} x {W}")
                pictures = {"frames_yuv": rng.integers(0, 256, (n_frames, H * 3 // 2, W), dtype=np.uint8),
                            "pixel_format": np.array(pixel_format)}
            np.savez(os.path.join(out, "clips", video, name + ".npz"), **pictures,
                     wav=(0.1 * rng.standard_normal((24000 if sample_rate is None else int(sample_rate)) * seconds)).astype(np.float32),
                     fps=np.float32(fps), **rate)
            lines.append(f"{video}/{name}.mp4")
        # a clip's first label row is start * DATA.TARGET_FPS (30 in both configurations), whatever rate the clip runs at
        rows = (nclips - 1) * seconds * 30 + n_frames if label_rows is None else int(label_rows)
        with open(os.path.join(out, "gaze_frame_label", f"{video}_frame_label.csv"), "w") as f:
            f.write(",".join(header) + "\n")
            for r in range(rows):
                xy = rng.random(2)
                lead = [str(r)] + ([f"{r / fps:.4f}"] if len(header) == 5 else [])
                f.write(",".join(lead + [f"{xy[0]:.6f}", f"{xy[1]:.6f}", str(int(rng.integers(0, 2)))]) + "\n")
    with open(os.path.join(out, "train.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out, "test.csv"), "w") as f:
        f.write("\n".join(lines[-int(test_clips):]) + "\n")
    return lines


def main(argv=None):
    p = argparse.ArgumentParser(description="Write a small random data set for CSTS_AMD.DATA_ROOT.")
    p.add_argument("--out", required=True, type=str)
    p.add_argument("--dataset", default="ego4d_av_gaze_forecast", choices=sorted(CLIP))
    p.add_argument("--videos", default=2, type=int)
    p.add_argument("--clips", default=3, type=int, help="clips per video")
    p.add_argument("--height", default=64, type=int)
    p.add_argument("--width", default=80, type=int)
    p.add_argument("--test-clips", default=2, type=int)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--sample-rate", default=None, type=int, help="write the waveforms at this rate with a sample_rate entry")
    p.add_argument("--pixel-format", default="rgb24", choices=("rgb24", "nv12", "i420"),
                   help="nv12 / i420: write frames_yuv (N, H * 3 / 2, W) with a pixel_format entry instead of frames_u8")
    a = p.parse_args(argv)
    if a.sample_rate is not None and a.sample_rate < 1:
        p.error("--sample-rate must be positive")
    lines = write_dataset(a.out, a.dataset, (a.clips,) * a.videos, ((a.height, a.width),), test_clips=a.test_clips, seed=a.seed,
                          sample_rate=a.sample_rate, pixel_format=a.pixel_format)
    print(f"wrote {len(lines)} clips of {a.dataset} to {a.out}")


if __name__ == "__main__":
    main()
