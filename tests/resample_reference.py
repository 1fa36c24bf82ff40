"""The rule of csts_resample_wav (include/csts_hip.h, csts_amd/inputs.py::resample_audio) restated in float64 numpy.  Not a test
module: tests/test_resample_host.py and tests/test_gpu_resample.py import it.

    up / down = target / rate reduced;  mx = max(up, down);  half = zeros * mx;  k = -half .. half
    h = sinc(k / mx) / mx * kaiser(2 half + 1, beta);  h = h / sum(h) * up
    n_out = ceil(n up / down);  y[m] = sum_i x[i] h[half + m down - i up]  over 0 <= i < n with the h index in [0, 2 half]

This is scipy.signal.resample_poly(x, up, down) with its defaults (zero extension, zero phase); nothing here imports scipy or
the package under test."""
import math

import numpy as np

RATES = (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 176400, 192000)
LENGTHS = (1, 2, 147, 1000, 4099)
TARGET = 24000


def ratio(rate, target=TARGET):
    g = math.gcd(int(rate), int(target))
    return int(target) // g, int(rate) // g


def design(rate, target=TARGET, zeros=10, beta=5.0):
    """-> (h float64 (2 half + 1,), up, down, half)."""
    up, down = ratio(rate, target)
    mx = max(up, down)
    half = zeros * mx
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(k / mx) / mx * np.kaiser(2 * half + 1, beta)
    return h / h.sum() * up, up, down, half


def out_len(n, up, down):
    return -(-int(n) * up // down)


def resample(x, h, up, down, half, m=None):
    """x float64 (n,) -> (y, K, S), each (n_out,): the outputs, the taps each one used and S = sum |x[i] h[.]|.
    m (optional): int64 output numbers; only those outputs are computed."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    n_out = out_len(n, up, down)
    m = np.arange(n_out, dtype=np.int64) if m is None else np.asarray(m, dtype=np.int64)
    lo = np.maximum(-((half - m * down) // up), 0)              # ceil((m down - half) / up), clipped to [0, n)
    hi = np.minimum((m * down + half) // up, n - 1)
    K = np.maximum(hi - lo + 1, 0)
    j = np.arange(int(K.max()), dtype=np.int64)
    i = lo[:, None] + j[None, :]
    ok = j[None, :] < K[:, None]
    t = half + m[:, None] * down - i * up
    prod = np.where(ok, x[np.where(ok, i, 0)] * h[np.where(ok, t, 0)], 0.0)
    return prod.sum(axis=1), K, np.abs(prod).sum(axis=1)


def downmix(wav):
    """(..., C, n) fp32 or int16 values -> the float64 mono signal the kernel filters: int16 scaled by 1 / 32768, channel mean."""
    w = np.asarray(wav)
    x = w.astype(np.float64) / 32768.0 if w.dtype == np.int16 else w.astype(np.float64)
    return x.mean(axis=-2)
