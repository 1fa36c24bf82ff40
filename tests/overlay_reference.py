"""The rule of csts_gaze_overlay (include/csts_hip.h) restated in float64 numpy, and the seeded cases of tests/test_gpu_overlay.py.
Not a test module: tests/test_overlay_host.py checks the cases on the CPU, tests/test_gpu_overlay.py compares the kernel with them.

cv2 is not a dependency of this project, so this restatement -- not cv2's resize / applyColorMap / addWeighted / circle -- is what
the kernel is held to."""
import functools

import numpy as np
import torch

CLOSE = 1e-3          # |v * 255 - nearest integer| up to which fp32 and float64 may quantise differently

# name -> (H, W, S, mh, mw, spatial_idx or None for the identity row)
CASES = {
    "identity_32": (32, 32, 32, 8, 8, None),
    "landscape_idx0": (36, 52, 32, 8, 8, 0),
    "landscape_idx1": (36, 52, 32, 8, 8, 1),
    "landscape_idx2": (36, 52, 32, 8, 8, 2),
    "byte_path_w50": (36, 50, 32, 8, 8, 1),
    "portrait": (52, 36, 32, 8, 8, 1),
    "map_7x9": (36, 52, 32, 7, 9, 1),
    "shipped_64x64": (270, 360, 256, 64, 64, 1),
}
N = 3
RADIUS = 5


def jet_formula(q):
    q4 = 4 * np.asarray(q, dtype=np.int64)
    return np.stack([np.clip(383 - np.abs(q4 - c), 0, 255) for c in (765, 510, 255)], axis=-1)


def params_row(H, W, S, spatial_idx):
    if spatial_idx is None:
        return [S, S, 0, 0, 0]
    from csts_amd import inputs
    return inputs.spatial_rule_host(np.zeros((1, 1, 2)), H, W, S, train=False, spatial_idx=spatial_idx)[0][0].tolist()


@functools.lru_cache(maxsize=None)
def make_case(name, seed=None):
    """frames uint8 (N, H, W, 3), maps fp32 (N, mh, mw) = min-max rescaled softmax(randn / 2), centers int32 (N, 2): frame 0 a
    marker inside the frame, frame 1 none (-1, -1), frame 2 one near the top right corner, clipped by the frame edge."""
    H, W, S, mh, mw, idx = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 100 if seed is None else seed)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    p = torch.softmax(torch.randn(N, mh * mw, generator=g) / 2, dim=-1)
    mn, mx = p.min(dim=-1, keepdim=True).values, p.max(dim=-1, keepdim=True).values
    maps = ((p - mn) / (mx - mn + 1e-6)).reshape(N, mh, mw).contiguous()
    centers = torch.tensor([[W // 2 - 3, H // 2 + 2], [-1, -1], [W - 2, 1]], dtype=torch.int32)
    return {"frames": frames, "maps": maps, "centers": centers, "row": params_row(H, W, S, idx), "S": S}


def _axis(E, ne, o, S, m):
    p = np.arange(E, dtype=np.int64)
    c = (2 * p + 1) * ne
    inside = (o * 2 * E <= c) & (c < (o + S) * 2 * E)
    cc = (p + 0.5) * ne / E - 0.5 - o
    src = np.maximum((cc + 0.5) * m / S - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), m - 1)
    i1 = np.minimum(i0 + 1, m - 1)
    return inside, i0, i1, src - i0


def reference(frames, maps, centers, row, S, alpha=0.4, radius=RADIUS):
    """float64.  Returns {"out" uint8 (N, H, W, 3), "q" (N, H, W), "heat" bool (N, H, W) = blended pixels, "close" bool = heat pixels
    whose v * 255 lies within CLOSE of an integer, "marker" bool}."""
    f = frames.numpy() if torch.is_tensor(frames) else np.asarray(frames)
    m = (maps.numpy() if torch.is_tensor(maps) else np.asarray(maps)).astype(np.float64)
    n, H, W, _ = f.shape
    mh, mw = m.shape[1:]
    nh, nw, y0, x0 = (int(v) for v in row[:4])
    cen = None if centers is None else (centers.numpy() if torch.is_tensor(centers) else np.asarray(centers)).astype(np.int64)
    iny, i0, i1, ly = _axis(H, nh, y0, S, mh)
    inx, j0, j1, lx = _axis(W, nw, x0, S, mw)
    top = m[:, i0][:, :, j0] * (1 - lx) + m[:, i0][:, :, j1] * lx
    bot = m[:, i1][:, :, j0] * (1 - lx) + m[:, i1][:, :, j1] * lx
    t = (top * (1 - ly)[None, :, None] + bot * ly[None, :, None]) * 255.0
    q = np.clip(np.floor(t).astype(np.int64), 0, 255)
    active = np.ones(n, dtype=bool) if cen is None else cen[:, 0] >= 0
    heat = (iny[:, None] & inx[None, :])[None] & active[:, None, None]
    close = heat & (np.abs(t - np.rint(t)) <= CLOSE)
    blend = np.rint((1.0 - alpha) * f.astype(np.float64) + alpha * jet_formula(q).astype(np.float64))
    out = np.where(heat[..., None], blend, f.astype(np.float64))
    marker = np.zeros((n, H, W), dtype=bool)
    if cen is not None:
        Y, X = np.arange(H, dtype=np.int64)[None, :, None], np.arange(W, dtype=np.int64)[None, None, :]
        d2 = (X - cen[:, 0, None, None]) ** 2 + (Y - cen[:, 1, None, None]) ** 2
        marker = (d2 <= radius * radius) & (cen[:, 0] >= 0)[:, None, None]
        out[marker] = (0.0, 255.0, 0.0)
    return {"out": out.astype(np.uint8), "q": q, "heat": heat, "close": close, "marker": marker}


@functools.lru_cache(maxsize=None)
def case_reference(name):
    c = make_case(name)
    return reference(c["frames"], c["maps"], c["centers"], c["row"], c["S"])


def compare(got, ref, what):
    """The bound of the overlay tests: exact outside the crop, on untouched frames, on marker pixels and on every blended pixel
    that is not close; a close pixel may be off by one JET step of 4 at alpha <= 0.4, i.e. by at most 2 a channel; close pixels
    are at most 1 % of the blended ones.  Prints the share and the count of differing pixels."""
    got = (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).astype(np.int64)
    want = ref["out"].astype(np.int64)
    loose = ref["close"] & ~ref["marker"]
    diff = np.abs(got - want).max(axis=-1)
    blended = int(ref["heat"].sum())
    share = float(ref["close"].sum()) / max(blended, 1)
    print(f"gaze_overlay {what}: {blended} blended pixels, close share {share:.4%}, pixels off by 1 or 2: "
          f"{int(((diff > 0) & (diff <= 2)).sum())}, off by more: {int((diff > 2).sum())}, off outside the close set: "
          f"{int(((diff > 0) & ~loose).sum())}")
    assert share <= 0.01, what
    assert int(diff[~loose].max(initial=0)) == 0, what
    assert int(diff[loose].max(initial=0)) <= 2, what
