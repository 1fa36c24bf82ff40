"""The colour rule of 4:2:0 frames (include/csts_hip.h), restated in numpy int64 for the tests: the tables recomputed from Kr and
Kb with exact rationals, the integer pixel rule, the two layouts (nearest chroma) and the real-valued matrix the rule rounds."""
from fractions import Fraction

import numpy as np

KR_KB = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}
FORMATS = ("nv12", "i420")
TABLES = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]


def rationals(matrix, full_range):
    """{sy, 2 sc (1 - Kr), -2 sc Kb (1 - Kb) / Kg, -2 sc Kr (1 - Kr) / Kg, 2 sc (1 - Kb)} as Fractions."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc = (Fraction(1), Fraction(1)) if full_range else (Fraction(255, 219), Fraction(255, 224))
    return [sy, 2 * sc * (1 - kr), -2 * sc * kb * (1 - kb) / kg, -2 * sc * kr * (1 - kr) / kg, 2 * sc * (1 - kb)]


def table(matrix, full_range):
    """{CY, CRV, CGU, CGV, CBU} = round(c * 2^20) (no coefficient lies on a half, so round() has no tie to break)."""
    return [int(round(c * (1 << 20))) for c in rationals(matrix, full_range)]


def pixels(Y, U, V, matrix="bt601", full_range=False):
    """The integer rule on arrays of equal shape -> uint8 (..., 3); also returns the largest accumulator magnitude."""
    cy, crv, cgu, cgv, cbu = table(matrix, full_range)
    y = Y.astype(np.int64) - (0 if full_range else 16)
    u, v = U.astype(np.int64) - 128, V.astype(np.int64) - 128
    acc = np.stack([cy * y + crv * v, cy * y + cgu * u + cgv * v, cy * y + cbu * u], axis=-1) + (1 << 19)
    return np.clip(acc >> 20, 0, 255).astype(np.uint8), int(np.abs(acc).max())


def real_pixels(Y, U, V, matrix="bt601", full_range=False):
    """clip(rint(real-valued matrix)) in float64 -> int64 (..., 3)."""
    c = [float(x) for x in rationals(matrix, full_range)]
    y = Y.astype(np.float64) - (0 if full_range else 16)
    u, v = U.astype(np.float64) - 128, V.astype(np.float64) - 128
    rgb = np.stack([c[0] * y + c[1] * v, c[0] * y + c[2] * u + c[3] * v, c[0] * y + c[4] * u], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.int64)


def planes(frames, pixel_format):
    """frames uint8 (..., H * 3 / 2, W) -> Y, U, V each (..., H, W): chroma sample (y >> 1, x >> 1) of pixel (y, x)."""
    rows, W = frames.shape[-2:]
    H = rows // 3 * 2
    assert rows * 2 == H * 3 and H % 2 == 0 and W % 2 == 0
    lead = frames.shape[:-2]
    Y = frames[..., :H, :]
    c = frames[..., H:, :]
    if pixel_format == "nv12":
        U, V = c[..., 0::2], c[..., 1::2]                                   # (..., H/2, W/2)
    else:
        c = c.reshape(lead + (2, H // 2, W // 2))
        U, V = c[..., 0, :, :], c[..., 1, :, :]
    up = lambda p: np.repeat(np.repeat(p, 2, axis=-2), 2, axis=-1)         # noqa: E731
    return Y, up(U), up(V)


def to_rgb(frames, pixel_format, matrix="bt601", full_range=False):
    """frames uint8 (..., H * 3 / 2, W) -> uint8 (..., H, W, 3) by the restated rule."""
    return pixels(*planes(np.asarray(frames), pixel_format), matrix, full_range)[0]


def all_triples(pixel_format):
    """Every (Y, U, V) byte triple exactly once, arranged as 256 frames of 128 x 512 pixels -> frames uint8 (256, 192, 512): frame n
    has U = n everywhere, chroma sample (cy, cx) of it has V = cx and the four pixels that share it carry Y = 4 cy + {0, 1, 2, 3}."""
    H, W = 128, 512
    cy, cx = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing="ij")
    frames = np.zeros((256, H * 3 // 2, W), np.uint8)
    for dy in range(2):
        for dx in range(2):
            frames[:, dy:H:2, dx::2] = (4 * cy + 2 * dy + dx).astype(np.uint8)
    U = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, H // 2, W // 2))
    V = np.broadcast_to(cx.astype(np.uint8), (256, H // 2, W // 2))
    if pixel_format == "nv12":
        frames[:, H:, 0::2] = U
        frames[:, H:, 1::2] = V
    else:
        frames[:, H:] = np.stack([U, V], axis=1).reshape(256, H // 2, W)
    return frames
