"""The rule of csts_attention_track (include/csts_hip.h) restated in numpy, and the seeded cases.  Not a test module:
tests/test_attention_track_host.py checks the restatement on the CPU, tests/test_gpu_attention_track.py compares the kernel with it.

The per-pair map and the mean are restated in np.float32 with the kernel's operation order: every step is one IEEE fp32
operation (no contraction in the kernel), so the result is comparable bit for bit.  The lattice extrema are taken in float64
through attention_reference.end_pixel_range / lattice_range."""
import functools
import math

import numpy as np
import torch

import attention_reference as A

F32 = np.float32

# name -> (Wn, heads, head_dim, T', h, w, T, S, F, seed, frames_idx (Wn, T)).  The smallest shapes at which the kernel can go wrong:
#   grid_6x6   frames hit 0, 1, 2 and 3 times, one index -1 and one >= F (both dropped), nobody hits the first five and the last
#              seven frames (empty runs at both ends of the offsets), a window whose frames are not ascending; T' = 3 under T = 6
#              takes both time clamps and the weights 1/4, 3/4;
#   grid_5x5   one head: the head mean is the head; a grid that is no multiple of anything;
#   shipped    the shipped grid and heads, the frames of a stride-18 plan with 9 frames between inputs: overlapping windows and
#              a tail past the recording's end;
#   wide_17x16 272 cells: more than the workgroup's 256 threads and no multiple of 4; T == T', the identity in time; a frame two
#              input frames of ONE window land on.
CASES = {
    "grid_6x6": (3, 2, 96, 3, 6, 6, 6, 48, 40, 1,
                 ((5, 8, 11, 14, 17, 20), (8, 11, 14, 17, 23, -1), (11, 14, 26, 29, 40, 32))),
    "grid_5x5": (2, 1, 96, 2, 5, 5, 4, 40, 12, 2, ((1, 3, 5, 7), (5, 7, 9, 10))),
    "shipped": (4, 8, 96, 4, 8, 8, 8, 256, 100, 3, tuple(tuple(18 * w + 9 * j for j in range(8)) for w in range(4))),
    "wide_17x16": (2, 2, 32, 4, 17, 16, 4, 96, 9, 4, ((0, 2, 4, 6), (4, 6, 8, 8))),
}


def frames_idx(name):
    return np.asarray(CASES[name][10], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the rule
def time_axis(j, T, Tp):
    """apa_axis(j, T, T') of fusion_maps.hip: (t0, t1, lambda fp32) from A = (2j + 1) T' - T, D = 2T in integers."""
    a, d = (2 * j + 1) * Tp - T, 2 * T
    t0, lam = 0, F32(0)
    if a > 0:
        q = a // d
        t0 = min(q, Tp - 1)
        lam = F32(a - q * d) / F32(d)
    return t0, min(t0 + 1, Tp - 1), lam


def with_head_mean(column):
    """fp32 (Wn, Hh, T', h, w) -> (Wn, Hh + 1, T', h, w): the heads, then ((0 + c_0) + c_1 + ...) / Hh in fp32."""
    col = np.asarray(column)
    assert col.dtype == F32
    s = np.zeros_like(col[:, 0])
    for k in range(col.shape[1]):
        s = s + col[:, k]
    return np.concatenate([col, (s / F32(col.shape[1]))[:, None]], axis=1)


def pair_map(cols, w, j, T):
    """m_p of pair (w, j) for every g: fl(fl((1 - lambda) col[t0]) + fl(lambda col[t1])), fp32 (Hh + 1, h, w)."""
    t0, t1, lam = time_axis(j, T, cols.shape[2])
    m = (F32(1) - lam) * cols[w, :, t0] + lam * cols[w, :, t1]
    assert m.dtype == F32
    return m


def pair_lists(idx, n_frames):
    """idx (Wn, T) -> for every output frame the pairs p = w T + j that land on it, ascending; frames outside [0, F) dropped."""
    flat = np.asarray(idx).reshape(-1)
    return [np.flatnonzero(flat == f) for f in range(int(n_frames))]


def order_offsets(idx, n_frames):
    """The device lists of csts_attention_track, built on the host: order int32 (P,) (the dropped pairs at its end), offsets
    int32 (F + 1,)."""
    lists = pair_lists(idx, n_frames)
    flat = np.asarray(idx).reshape(-1)
    dropped = np.flatnonzero((flat < 0) | (flat >= n_frames))
    order = np.concatenate(lists + [dropped]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    assert order.shape[0] == flat.shape[0]
    return order, offsets


def mean_maps(column, idx, n_frames):
    """-> mixed fp32 (F, Hh + 1, h, w) = (((0 + m_p0) + m_p1) + ...) * (1 / n) in list order, 0 where n == 0; count int32 (F,)."""
    cols = with_head_mean(column)
    T = np.asarray(idx).shape[1]
    lists = pair_lists(idx, n_frames)
    mixed = np.zeros((int(n_frames),) + cols.shape[1:2] + cols.shape[3:], dtype=F32)
    count = np.zeros(int(n_frames), dtype=np.int32)
    for f, pairs in enumerate(lists):
        acc = np.zeros_like(mixed[f])
        for p in pairs:
            acc = acc + pair_map(cols, int(p) // T, int(p) % T, T)
        if len(pairs):
            acc = acc * (F32(1) / F32(len(pairs)))
        assert acc.dtype == F32
        mixed[f], count[f] = acc, len(pairs)
    return mixed, count


def lattice_extrema(mixed, S):
    """float64 (lo, hi) of the bilinear upsample of fp32 maps (..., h, w) over the S x S lattice, from the end pixels: (..., 2)."""
    lo, hi = A.end_pixel_range(np.asarray(mixed, dtype=np.float64), S)
    return np.stack([lo, hi], axis=-1)


def rescale(mixed, rng):
    """maps = (mixed - lo) / (hi - lo + 1e-6) in fp32 from an fp32 range (..., 2)."""
    rng = np.asarray(rng)
    assert mixed.dtype == F32 and rng.dtype == F32
    lo, hi = rng[..., 0, None, None], rng[..., 1, None, None]
    return (mixed - lo) / (hi - lo + F32(1e-6))


# ------------------------------------------------------------------------------------------------ seeded cases
@functools.lru_cache(maxsize=None)
def host_column(name):
    """fp32 (Wn, Hh, T', h, w), softmax-like and positive: attention_reference.host_column's recipe on this case's shape."""
    Wn, Hh, _, Tp, h, w, _, _, _, seed, _ = CASES[name]
    g = torch.Generator().manual_seed(3000 + seed)
    z = 2.0 * torch.randn(Wn, Hh, Tp, h * w, h * w + 1, generator=g, dtype=torch.float64)
    return torch.softmax(z, dim=-1)[..., -1].reshape(Wn, Hh, Tp, h, w).numpy().astype(F32)


@functools.lru_cache(maxsize=None)
def kernel_inputs(name):
    """Packed qkv fp32 (Wn, N, 3C) and lse fp32 (Wn, Hh, N) of the spatial fusion block, attention_reference.kernel_case's recipe
    (random rows, q scaled so the logits are about 2 randn, the float64 log-sum-exp under the spatial mask, log2 domain) on this
    case's shape: ops.audio_pixel_attn turns them into the `column` the track is built from, and into the one-clip maps a frame
    with one pair must equal."""
    Wn, Hh, hd, Tp, h, w, _, _, _, seed, _ = CASES[name]
    HW = h * w
    N, C = Tp * HW + Tp, Hh * hd
    g = torch.Generator().manual_seed(4000 + seed)
    qkv = torch.randn(Wn, N, 3 * C, generator=g)
    qkv[:, :, :C] *= 2.0
    x = qkv.double().reshape(Wn, N, 3, Hh, hd)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    z2 = (q @ k.transpose(-2, -1)) * (hd ** -0.5 * math.log2(math.e))
    z2 = z2.masked_fill(~A.spatial_mask(Tp, HW), -float("inf"))
    lse2 = torch.logsumexp(z2 * math.log(2.0), dim=-1) / math.log(2.0)
    return {"qkv": qkv, "lse": lse2.float()}
