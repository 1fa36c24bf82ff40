"""The rule of csts_audio_pixel_attn (include/csts_hip.h) restated in float64 numpy, the reference's own order
(slowfast/visualization/visualization.py:189-216: slice, stack, trilinear upsample, per-frame min-max, astype(uint8)) stated in
torch, and the seeded cases.  Not a test module: tests/test_attention_maps_host.py checks the cases on the CPU,
tests/test_gpu_audio_pixel_attn.py compares the kernel with them.

The quantised value follows the convention of tests/overlay_reference.py: q = floor(255 v), and two statements of the rule may
differ by one step only where float64 255 v lies within CLOSE of an integer."""
import functools
import math
import os

import numpy as np
import torch

CLOSE = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (B, heads, head_dim, T', h, w, T, S, seed).  The smallest shapes that take every index path of the kernel: the shipped
# grid; an odd grid with T' = 3 (time weights 1/4, 3/4 and both clamps) and two heads; one head (the mean is the head), a 5 x 5
# grid that is no multiple of anything and three clips; T == T', the identity in time.  The seeds are ones for which the float64
# restatement alone keeps the close set under the 1 % cap of the picture comparison (a frame's minimum quantises to exactly 0,
# so on a small crop the clamped corner that holds it is already a percent of the frame): the cap is a condition of the cases.
CASES = {
    "shipped": (2, 8, 96, 4, 8, 8, 8, 256, 0),
    "grid_6x6": (1, 2, 96, 3, 6, 6, 6, 48, 1),
    "grid_5x5": (3, 1, 96, 2, 5, 5, 4, 40, 1),
    "time_identity": (1, 2, 96, 4, 6, 6, 4, 48, 4),
}


# ------------------------------------------------------------------------------------------------ the rule, float64
def axis(S, m):
    """Lattice points 0 .. S - 1 on an axis of m cells (align_corners=False): (i0, i1, lambda)."""
    p = np.arange(S, dtype=np.float64)
    src = np.maximum((p + 0.5) * m / S - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), m - 1)
    i1 = np.minimum(i0 + 1, m - 1)
    return i0, i1, src - i0


def head_mean(column):
    """(B, Hh, T', h, w) -> (B, Hh + 1, T', h, w) float64: the heads, then their mean."""
    c = np.asarray(column, dtype=np.float64)
    return np.concatenate([c, c.mean(axis=1, keepdims=True)], axis=1)


def mix_time(maps, T):
    """(..., T', h, w) -> (..., T, h, w): m_j = (1 - lambda) col[t0] + lambda col[t1]."""
    c = np.asarray(maps, dtype=np.float64)
    t0, t1, lam = axis(T, c.shape[-3])
    lam = lam[:, None, None]
    return (1.0 - lam) * c[..., t0, :, :] + lam * c[..., t1, :, :]


def upsample(m, S):
    """(..., h, w) -> (..., S, S): the bilinear sample on the crop lattice."""
    i0, i1, ly = axis(S, m.shape[-2])
    j0, j1, lx = axis(S, m.shape[-1])
    top = m[..., i0, :][..., j0] + lx * (m[..., i0, :][..., j1] - m[..., i0, :][..., j0])
    bot = m[..., i1, :][..., j0] + lx * (m[..., i1, :][..., j1] - m[..., i1, :][..., j0])
    return top + ly[:, None] * (bot - top)       # a + l (b - a), the kernel's form: a clamped border (b == a) stays a exactly


def end_pixels(S, m):
    """The first and last lattice point of every run that shares the lower cell i0."""
    i0 = axis(S, m)[0]
    first = np.flatnonzero(np.concatenate([[True], i0[1:] != i0[:-1]]))
    last = np.flatnonzero(np.concatenate([i0[1:] != i0[:-1], [True]]))
    return np.unique(np.concatenate([first, last]))


def lattice_range(m, S):
    """(lo, hi) of the upsample over the whole S x S lattice, each (...,)."""
    v = upsample(m, S)
    return v.min(axis=(-2, -1)), v.max(axis=(-2, -1))


def end_pixel_range(m, S):
    """(lo, hi) from the end pixels alone: at most 2h x 2w samples."""
    v = upsample(m, S)[..., end_pixels(S, m.shape[-2]), :][..., end_pixels(S, m.shape[-1])]
    return v.min(axis=(-2, -1)), v.max(axis=(-2, -1))


def restate(column, T, S):
    """column (B, Hh, T', h, w) -> the outputs of the kernel in float64: {"column_mean" (B, T', h, w), "maps" (B, Hh + 1, T, h, w),
    "range" (B, Hh + 1, T, 2)} and, for the comparison of pictures, "t" (B, Hh + 1, T, S, S) = 255 * upsample(maps), "q" =
    clip(floor(t), 0, 255), "close" = |t - rint(t)| <= CLOSE."""
    cols = head_mean(column)
    m = mix_time(cols, T)
    lo, hi = end_pixel_range(m, S)
    maps = (m - lo[..., None, None]) / (hi - lo + 1e-6)[..., None, None]
    t = upsample(maps, S) * 255.0
    return {"column_mean": cols[:, -1], "maps": maps, "range": np.stack([lo, hi], axis=-1), "mixed": m, "t": t,
            "q": np.clip(np.floor(t).astype(np.int64), 0, 255), "close": np.abs(t - np.rint(t)) <= CLOSE}


# ------------------------------------------------------------------------------------------------ the reference's order, torch
def reference_order(column, T, S):
    """visualization.py:189-216 on the stacked slices `column` (B, Heads, T', h, w), as the reference runs it (fp32): trilinear
    upsample to (T, S, S), then per frame (x - min) / (max - min + 1e-6) * 255 and astype(uint8).  -> int64 (B, Heads, T, S, S)."""
    x = torch.as_tensor(np.asarray(column), dtype=torch.float32)
    up = torch.nn.functional.interpolate(x, size=(T, S, S), mode="trilinear", align_corners=False).numpy()
    lo = up.min(axis=(-2, -1), keepdims=True)
    hi = up.max(axis=(-2, -1), keepdims=True)
    return ((up - lo) / (hi - lo + 1e-6) * 255).astype(np.uint8).astype(np.int64)


# ------------------------------------------------------------------------------------------------ seeded cases
@functools.lru_cache(maxsize=None)
def host_column(name):
    """float64 (B, Hh, T', h, w): softmax(2 randn) over the hw + 1 keys a video token of the spatial fusion block sees (its
    frame's tokens and that frame's audio token, the last one), of which the audio key's probability is the column."""
    B, Hh, _, Tp, h, w, _, _, seed = CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    z = 2.0 * torch.randn(B, Hh, Tp, h * w, h * w + 1, generator=g, dtype=torch.float64)
    return torch.softmax(z, dim=-1)[..., -1].reshape(B, Hh, Tp, h, w).numpy()


@functools.lru_cache(maxsize=None)
def fixture_column():
    """The column cut from the reference's own probabilities (tests/golden/model_T8_B1_attn.npz), (1, 8, 4, 8, 8) float64."""
    attn = np.load(os.path.join(GOLDEN, "model_T8_B1_attn.npz"))["spatial_attn"].astype(np.float64)
    return cut_column(attn, 4, 64).reshape(1, attn.shape[1], 4, 8, 8)


def cut_column(attn, Tp, HW):
    """attn (B, Hh, N, N) -> (B, Hh, T', HW): attn[:, :, HW t : HW (t + 1), T' HW + t], visualization.py:190."""
    return np.stack([attn[:, :, HW * t:HW * (t + 1), Tp * HW + t] for t in range(Tp)], axis=2)


def spatial_mask(Tp, HW):
    """bool (N, N): True where av_attention.py:337-346 lets query and key see each other."""
    N = Tp * HW + Tp
    frame = np.concatenate([np.repeat(np.arange(Tp), HW), np.arange(Tp)])
    return torch.from_numpy(frame[:, None] == frame[None, :]).reshape(N, N)


@functools.lru_cache(maxsize=None)
def kernel_case(name, half=None):
    """Random packed qkv of the spatial fusion block and everything the kernel test holds the kernel to, computed ONCE per case
    in float64 torch on the CPU.  half: None (fp32) or a torch 16-bit dtype; the float64 side then starts from the rounded
    values, so the difference is the kernel's arithmetic alone.  q is scaled so the logits are about 2 randn.
    -> {"qkv" (B, N, 3C), "lse" fp32 (B, Hh, N) log2 domain with the spatial mask, "column" float64 (B, Hh, T', h, w)}."""
    B, Hh, hd, Tp, h, w, _, _, seed = CASES[name]
    HW = h * w
    N, C = Tp * HW + Tp, Hh * hd
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    qkv[:, :, :C] *= 2.0
    if half is not None:
        qkv = qkv.to(half)
    x = qkv.double().reshape(B, N, 3, Hh, hd)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    z2 = (q @ k.transpose(-2, -1)) * (hd ** -0.5 * math.log2(math.e))                 # log2-domain logits (B, Hh, N, N)
    z2 = z2.masked_fill(~spatial_mask(Tp, HW), -float("inf"))
    lse2 = torch.logsumexp(z2 * math.log(2.0), dim=-1) / math.log(2.0)
    probs = torch.exp2(z2 - lse2[..., None]).numpy()
    return {"qkv": qkv, "lse": lse2.float(), "column": cut_column(probs, Tp, HW).reshape(B, Hh, Tp, h, w)}
