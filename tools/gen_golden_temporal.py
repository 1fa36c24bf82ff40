#!/usr/bin/env python3
"""Write tests/golden/temporal_sampling.npz by RUNNING THE REFERENCE's temporal sampling.

Build-container tooling only (needs the reference checkout; never runs on the GPU box, never imported by the product):

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_temporal.py --reference DIR     (DIR: a checkout of the reference)

slowfast/datasets/decoder.py is imported unmodified from the reference, with an import-only stub for torchvision.io (it is
never called on this path), the way tools/gen_golden_spatial.py imports the spatial transforms.  Each case runs the tail of
decode() on a fully decoded video (decoder.py:396-411): the clip size of the call, get_start_end_idx, then temporal_sampling
of the frame numbers 0 .. video_size - 1 -- the `frames_idx` the datasets use.  random is seeded; random.uniform is wrapped
only to RECORD the variate each draw consumed (peeked from the generator state, then the real call runs).  Stored per case:
the inputs, start, end, the sampled frame numbers and the variate (0 where the reference drew none)."""
import argparse
import importlib
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "temporal_sampling.npz")


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference(ref_root):
    """slowfast.datasets.decoder from the reference tree, without running the packages' __init__."""
    _mod("torchvision")
    sys.modules["torchvision"].io = _mod("torchvision.io")
    pkg = os.path.join(ref_root, "slowfast")
    _mod("slowfast", __path__=[pkg])
    _mod("slowfast.datasets", __path__=[os.path.join(pkg, "datasets")])
    return importlib.import_module("slowfast.datasets.decoder")


class Recorder:
    def __init__(self):
        self.real_uniform = random.uniform
        self.u, self.drawn = 0.0, False

    def uniform(self, a, b):
        state = random.getstate()
        u = random.random()                      # the double the draw below consumes (uniform = a + (b - a) * random())
        random.setstate(state)
        r = self.real_uniform(a, b)
        assert r == a + (b - a) * u and not self.drawn, (r, a, b, u)
        self.u, self.drawn = u, True
        return r

    def __enter__(self):
        random.uniform = self.uniform
        return self

    def __exit__(self, *exc):
        random.uniform = self.real_uniform


CASES = [
    # name, video_size, num_frames, sampling_rate, clip_idx, num_clips, target_fps, fps, use_offset
    ("ego4d_test_clip", 86, 8, 8, 1, 1, 30, 30, False),          # 22, 31, ..., 85
    ("ego4d_first_clip", 86, 8, 8, 0, 1, 30, 30, False),
    ("ego4d_estimation", 150, 8, 8, 0, 1, 30, 30, False),
    ("aria_T32", 60, 32, 4, 1, 1, 20, 20, False),                # the clip is longer than the video: the clamp is active
    ("aria_T8", 60, 8, 4, 1, 1, 20, 20, False),
    ("offset_1_clip", 150, 8, 8, 0, 1, 30, 30, True),
    ("offset_3_clips_0", 151, 8, 8, 0, 3, 30, 30, True),
    ("offset_3_clips_1", 151, 8, 8, 1, 3, 30, 30, True),
    ("offset_3_clips_2", 151, 8, 8, 2, 3, 30, 30, True),
    ("ten_views_3", 300, 8, 8, 3, 10, 30, 30, False),            # fractional start
    ("ten_views_7", 301, 16, 4, 7, 10, 30, 30, False),
    ("short_video", 40, 8, 8, 1, 1, 30, 30, False),              # shorter than the clip
    ("short_video_T16", 17, 16, 8, 0, 2, 30, 30, False),
    ("fps_25", 125, 8, 8, 1, 1, 30, 25, False),                  # fps != target_fps: a fractional clip size
    ("fps_60", 300, 8, 8, 1, 2, 30, 60, False),
    ("fps_24_T16", 200, 16, 4, 2, 5, 30, 24, True),
] + [(f"random_{i}", (97, 150, 86, 300, 61)[i % 5], (8, 16)[i % 2], (8, 4, 2)[i % 3], -1, 1, 30, (30, 25)[i % 4 == 3], False)
     for i in range(20)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CSTS_REFERENCE"), help="checkout of the reference repository")
    args = ap.parse_args()
    if not args.reference or not os.path.isfile(os.path.join(args.reference, "slowfast", "datasets", "decoder.py")):
        ap.error("--reference DIR (or CSTS_REFERENCE) must name a checkout of the reference repository")
    decoder = import_reference(args.reference)
    arrays, meta = {}, []
    for ci, (name, size, T, rate, idx, nclips, tfps, fps, offset) in enumerate(CASES):
        random.seed(3000 + ci)
        clip_sz = ((rate + 1) * (T - 1) + 1) / tfps * fps                    # decoder.py:397
        with Recorder() as rec:
            start, end = decoder.get_start_end_idx(size, clip_sz, idx, nclips, use_offset=offset)
        assert rec.drawn == (idx == -1)
        index = decoder.temporal_sampling(torch.arange(size), start, end, T)
        p = f"c{ci}_"
        arrays.update({p + "start": np.float64(start), p + "end": np.float64(end), p + "u": np.float64(rec.u),
                       p + "index": index.numpy().astype(np.int64)})
        meta.append({"name": name, "video_size": size, "num_frames": T, "sampling_rate": rate, "clip_idx": idx,
                     "num_clips": nclips, "target_fps": tfps, "fps": fps, "use_offset": offset})
        print(f"{name:18s} start {start!r:22} end {end!r:22} {index.tolist()}")
    arrays["cases"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
