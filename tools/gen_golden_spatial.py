#!/usr/bin/env python3
"""Write tests/golden/spatial_sampling.npz by RUNNING THE REFERENCE's spatial sampling.

Build-container tooling only (needs the reference checkout; never runs on the GPU box, never imported by the product):

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_spatial.py --reference DIR     (DIR: a checkout of the reference)

slowfast/datasets/utils.py and transform.py are imported unmodified from the reference, with import-only stubs for the
packages they import but never call on this path (torchvision, cv2, ipdb, the path manager), the way oracle/gen_golden.py
imports the model.  Each case runs the dataset's own sequence (ego4d_avgaze_forecast.py:294-311): tensor_normalize, permute
to C T H W, spatial_sampling(..., gaze_loc=label).  np.random is seeded; np.random.uniform is wrapped only to RECORD the
variate each draw consumed (peeked from the generator state, then the real call runs) and which step drew it;
transform.random_short_side_scale_jitter is wrapped only to record the resized clip, from which the crop offsets and the flip
are read back by exact matching.  Stored per case: uint8 frames, labels, the variates u0..u3 (0 where the reference drew none),
the observed params (new h, new w, y0, x0, flip), the output frames and the output labels."""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "spatial_sampling.npz")
MEAN, STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference(ref_root):
    """slowfast.datasets.{transform, utils} from the reference tree, without running the packages' __init__ (which imports
    every dataset and their decoders)."""
    for n in ("ipdb", "cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
        _mod(n)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    pkg = os.path.join(ref_root, "slowfast")
    _mod("slowfast", __path__=[pkg])
    _mod("slowfast.utils", __path__=[os.path.join(pkg, "utils")])
    _mod("slowfast.utils.env", pathmgr=None)
    _mod("slowfast.datasets", __path__=[os.path.join(pkg, "datasets")])
    transform = importlib.import_module("slowfast.datasets.transform")
    utils = importlib.import_module("slowfast.datasets.utils")
    return transform, utils


class Recorder:
    SLOT = {"random_short_side_scale_jitter": 0, "horizontal_flip_gaze": 3}

    def __init__(self, transform):
        self.real_uniform = np.random.uniform
        self.real_jitter = transform.random_short_side_scale_jitter
        self.transform = transform
        self.u = np.zeros(4)
        self.drawn = np.zeros(4, dtype=bool)
        self.resized = None

    def uniform(self, low=0.0, high=1.0, size=None):
        assert size is None
        state = np.random.get_state()
        u = np.random.random_sample()            # the double the draw below consumes (legacy uniform = low + (high - low) u)
        np.random.set_state(state)
        r = self.real_uniform(low, high)
        assert r == low + (high - low) * u, (r, low, high, u)
        caller = sys._getframe(1)
        name = caller.f_code.co_name
        slot = self.SLOT.get(name)
        if name == "random_crop_gaze":
            slot = 2 if "sort_gaze_y" in caller.f_locals else 1
        assert slot is not None and not self.drawn[slot], name
        self.u[slot], self.drawn[slot] = u, True
        return r

    def jitter(self, *a, **k):
        images, boxes = self.real_jitter(*a, **k)
        self.resized = images.clone()
        return images, boxes

    def __enter__(self):
        np.random.uniform = self.uniform
        self.transform.random_short_side_scale_jitter = self.jitter
        return self

    def __exit__(self, *exc):
        np.random.uniform = self.real_uniform
        self.transform.random_short_side_scale_jitter = self.real_jitter


def observed_params(resized, out, S):
    """(new h, new w, y0, x0, flip) such that resized[..., y0:y0+S, x0:x0+S] (mirrored if flip) == out exactly; unique."""
    _, _, nh, nw = resized.shape
    hits = []
    for flip in (0, 1):
        o = out.flip(-1) if flip else out
        for y0 in range(nh - S + 1):
            for x0 in range(nw - S + 1):
                if torch.equal(resized[:, :, y0:y0 + S, x0:x0 + S], o):
                    hits.append((nh, nw, y0, x0, flip))
    assert len(hits) == 1, hits
    return hits[0]


S = 16          # small clips: the fixture stays a few hundred kB (realistic sizes are checked on the GPU against the definition)
CASES = [
    # name, H, W, T, train, min, max, spatial_idx, random_flip, inverse_uniform, labels
    ("landscape", 20, 28, 4, True, 16, 20, -1, True, False, "inside"),
    ("landscape_b", 20, 28, 4, True, 16, 20, -1, True, False, "inside"),
    ("portrait", 28, 20, 4, True, 16, 20, -1, True, False, "inside"),
    ("portrait_noflip", 28, 20, 4, True, 16, 20, -1, False, False, "inside"),
    ("square", 24, 24, 4, True, 18, 22, -1, True, False, "inside"),
    ("square_eq_crop", 16, 16, 4, True, 16, 16, -1, True, False, "outside"),
    ("size_eq_short", 18, 25, 4, True, 18, 18, -1, True, False, "inside"),
    ("spread_x", 18, 40, 8, True, 17, 19, -1, True, False, "spread_x"),
    ("spread_y", 40, 18, 8, True, 17, 19, -1, True, False, "spread_y"),
    ("spread_xy", 20, 20, 8, True, 19, 22, -1, False, False, "spread_xy"),
    ("outside", 20, 30, 8, True, 17, 21, -1, True, False, "outside_mixed"),
    ("inverse_uniform", 22, 30, 4, True, 16, 24, -1, True, True, "inside"),
    ("test0_landscape", 20, 30, 4, False, 16, 16, 0, True, False, "inside"),
    ("test1_landscape", 20, 30, 4, False, 16, 16, 1, True, False, "outside"),
    ("test2_landscape", 20, 30, 4, False, 16, 16, 2, True, False, "inside"),
    ("test0_portrait", 30, 20, 4, False, 16, 16, 0, True, False, "inside"),
    ("test1_portrait", 30, 20, 4, False, 16, 16, 1, True, False, "inside"),
    ("test2_portrait", 30, 20, 4, False, 16, 16, 2, True, False, "outside"),
]


def make_labels(kind, T, rng):
    lab = np.zeros((T, 3))
    lab[:, 2] = rng.integers(0, 3, T)            # an extra column (fixation type), copied through
    if kind == "inside":
        lab[:, :2] = rng.uniform(0.05, 0.95, (T, 2))
    elif kind == "outside":                      # points over [-0.3, 1.3], two of them surely outside
        lab[:, :2] = rng.uniform(-0.3, 1.3, (T, 2))
        lab[0, 0], lab[1, 1] = -0.2, 1.25
    elif kind == "outside_mixed":                # a few points outside among inside ones
        lab[:, :2] = rng.uniform(0.2, 0.8, (T, 2))
        lab[0, 0], lab[3, 0], lab[5, 1] = -0.15, 1.1, 1.2
    else:
        lab[:, :2] = rng.uniform(0.3, 0.7, (T, 2))
        spread = np.linspace(0.02, 0.98, T)
        rng.shuffle(spread)
        if kind in ("spread_x", "spread_xy"):
            lab[:, 0] = spread
        if kind in ("spread_y", "spread_xy"):
            lab[:, 1] = spread[::-1].copy()
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CSTS_REFERENCE"), help="checkout of the reference repository")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, "slowfast", "datasets")):
        ap.error("--reference DIR (or CSTS_REFERENCE) must name a checkout of the reference repository")
    transform, utils = import_reference(args.reference)
    rng = np.random.default_rng(20261015)
    arrays, meta = {}, []
    for ci, (name, H, W, T, train, mn, mx, idx, flip, inv, kind) in enumerate(CASES):
        np.random.seed(1000 + ci)
        u8 = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
        lab = make_labels(kind, T, rng)
        frames = utils.tensor_normalize(torch.from_numpy(u8), MEAN, STD).permute(3, 0, 1, 2)
        with Recorder(transform) as rec:
            out, out_lab = utils.spatial_sampling(frames, gaze_loc=lab.copy(), spatial_idx=idx, min_scale=mn, max_scale=mx,
                                                  crop_size=S, random_horizontal_flip=flip, inverse_uniform_sampling=inv)
        assert tuple(out.shape) == (3, T, S, S), out.shape
        params = observed_params(rec.resized, out, S)
        p = f"c{ci}_"
        arrays.update({p + "frames": u8, p + "labels": lab, p + "u": rec.u, p + "drawn": rec.drawn,
                       p + "params": np.array(params, dtype=np.int32), p + "out": out.numpy().astype(np.float32),
                       p + "out_labels": np.asarray(out_lab, dtype=np.float64)})
        meta.append({"name": name, "H": H, "W": W, "T": T, "S": S, "train": train, "min_scale": mn, "max_scale": mx,
                     "spatial_idx": idx, "random_flip": flip, "inverse_uniform": inv})
        print(f"{name:18s} params {params} drawn {rec.drawn.astype(int).tolist()}")
    arrays["cases"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB, {len(CASES)} cases")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
