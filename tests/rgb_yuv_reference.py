"""The inverse colour rule, rgb_to_yuv (include/csts_hip.h), restated in numpy int64 for the tests: the nine coefficients of every
(matrix, range) recomputed from Kr and Kb with exact rationals, the integer luma and chroma rules, the two layouts, the real-valued
matrix the rule rounds, and the `where` composition that states what the 4:2:0 overlay writes."""
from fractions import Fraction

import numpy as np

from yuv_reference import KR_KB, FORMATS, TABLES  # noqa: F401


def rationals(matrix, full_range):
    """{ty Kr, ty Kg, ty Kb | -tc Kr / (2 (1 - Kb)), -tc Kg / (2 (1 - Kb)), tc / 2 | tc / 2, -tc Kg / (2 (1 - Kr)),
    -tc Kb / (2 (1 - Kr))} as Fractions, ty = 219/255 and tc = 224/255 (limited) or 1 (full)."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ty, tc = (Fraction(1), Fraction(1)) if full_range else (Fraction(219, 255), Fraction(224, 255))
    return [ty * kr, ty * kg, ty * kb,
            -tc * kr / (2 * (1 - kb)), -tc * kg / (2 * (1 - kb)), tc / 2,
            tc / 2, -tc * kg / (2 * (1 - kr)), -tc * kb / (2 * (1 - kr))]


def table(matrix, full_range):
    """round(c * 2^20) of the nine rationals, half away from zero (exact: Fractions)."""
    out = []
    for c in rationals(matrix, full_range):
        v = c * (1 << 20)
        out.append(int(v + Fraction(1, 2)) if v >= 0 else -int(-v + Fraction(1, 2)))
    return out


def luma(rgb, matrix="bt601", full_range=False):
    """rgb integer (..., 3) -> int64 (...): the luma rule; also returns the largest accumulator magnitude."""
    yr, yg, yb = table(matrix, full_range)[:3]
    p = rgb.astype(np.int64)
    acc = yr * p[..., 0] + yg * p[..., 1] + yb * p[..., 2] + (1 << 19)
    return np.clip((acc >> 20) + (0 if full_range else 16), 0, 255), int(np.abs(acc).max())


def chroma(sums, matrix="bt601", full_range=False):
    """sums integer (..., 3) = the four pixels of a block added per channel -> U, V int64 (...) and the largest accumulator."""
    t = table(matrix, full_range)
    s = sums.astype(np.int64)
    au = t[3] * s[..., 0] + t[4] * s[..., 1] + t[5] * s[..., 2] + (1 << 21)
    av = t[6] * s[..., 0] + t[7] * s[..., 1] + t[8] * s[..., 2] + (1 << 21)
    return np.clip((au >> 22) + 128, 0, 255), np.clip((av >> 22) + 128, 0, 255), int(max(np.abs(au).max(), np.abs(av).max()))


def block_sums(rgb):
    """rgb (..., H, W, 3) -> int64 (..., H / 2, W / 2, 3): the box filter."""
    p = rgb.astype(np.int64)
    return p[..., 0::2, 0::2, :] + p[..., 0::2, 1::2, :] + p[..., 1::2, 0::2, :] + p[..., 1::2, 1::2, :]


def pack(Y, U, V, pixel_format):
    """Y (..., H, W), U and V (..., H / 2, W / 2) -> frames uint8 (..., H * 3 / 2, W)."""
    H, W = Y.shape[-2:]
    lead = Y.shape[:-2]
    if pixel_format == "nv12":
        c = np.stack([U, V], axis=-1).reshape(lead + (H // 2, W))
    else:
        c = np.stack([U, V], axis=-3).reshape(lead + (H // 2, W))
    return np.concatenate([Y, c], axis=-2).astype(np.uint8)


def to_yuv(rgb, pixel_format, matrix="bt601", full_range=False):
    """rgb uint8 (..., H, W, 3), H and W even -> frames uint8 (..., H * 3 / 2, W) by the restated rule."""
    rgb = np.asarray(rgb)
    Y = luma(rgb, matrix, full_range)[0]
    U, V, _ = chroma(block_sums(rgb), matrix, full_range)
    return pack(Y, U, V, pixel_format)


def real_yuv(rgb, sums, matrix="bt601", full_range=False):
    """floor(real-valued matrix + 0.5), clipped, in float64: luma of rgb (..., 3) and U, V of sums (..., 3) / 4."""
    c = [float(x) for x in rationals(matrix, full_range)]
    p, s = rgb.astype(np.float64), sums.astype(np.float64) / 4.0
    Y = np.floor(c[0] * p[..., 0] + c[1] * p[..., 1] + c[2] * p[..., 2] + 0.5) + (0 if full_range else 16)
    U = np.floor(c[3] * s[..., 0] + c[4] * s[..., 1] + c[5] * s[..., 2] + 0.5) + 128
    V = np.floor(c[6] * s[..., 0] + c[7] * s[..., 1] + c[8] * s[..., 2] + 0.5) + 128
    return [np.clip(x, 0, 255).astype(np.int64) for x in (Y, U, V)]


def triple_frames(r0, r1):
    """Every (R, G, B) with R in [r0, r1) as 2 x 2 blocks of four equal pixels: rgb uint8 (r1 - r0, 512, 512, 3); frame i has
    R = r0 + i everywhere, block (cy, cx) of it has G = cy and B = cx."""
    n = r1 - r0
    rgb = np.empty((n, 512, 512, 3), np.uint8)
    rgb[..., 0] = np.arange(r0, r1, dtype=np.uint8)[:, None, None]
    rgb[..., 1] = np.repeat(np.arange(256, dtype=np.uint8), 2)[None, :, None]
    rgb[..., 2] = np.repeat(np.arange(256, dtype=np.uint8), 2)[None, None, :]
    return rgb


def split(frames, pixel_format):
    """frames uint8 (..., H * 3 / 2, W) -> Y (..., H, W), U, V (..., H / 2, W / 2) (views where the layout allows)."""
    rows, W = frames.shape[-2:]
    H = rows // 3 * 2
    lead = frames.shape[:-2]
    c = frames[..., H:, :]
    if pixel_format == "nv12":
        return frames[..., :H, :], c[..., 0::2], c[..., 1::2]
    c = c.reshape(lead + (2, H // 2, W // 2))
    return frames[..., :H, :], c[..., 0, :, :], c[..., 1, :, :]


def compose(frames, D, M, pixel_format, matrix="bt601", full_range=False):
    """What the 4:2:0 overlay writes: where(M, rgb_to_yuv(D), frames) with frames uint8 (N, H * 3 / 2, W), D uint8 (N, H, W, 3) the
    RGB overlay of yuv_to_rgb(frames) and M bool (N, H, W) the drawn mask, taken per pixel for luma and per 2 x 2 block (any) for
    chroma.  Also returns the per-block count of drawn pixels (N, H / 2, W / 2)."""
    frames, D, M = np.asarray(frames), np.asarray(D), np.asarray(M)
    enc = to_yuv(D, pixel_format, matrix, full_range)
    Y0, U0, V0 = split(frames, pixel_format)
    Y1, U1, V1 = split(enc, pixel_format)
    cnt = M[:, 0::2, 0::2].astype(np.int64) + M[:, 0::2, 1::2] + M[:, 1::2, 0::2] + M[:, 1::2, 1::2]
    blk = cnt > 0
    return pack(np.where(M, Y1, Y0), np.where(blk, U1, U0), np.where(blk, V1, V0), pixel_format), cnt
