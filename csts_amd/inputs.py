"""On-device input pipeline: the steps the reference runs on the CPU right before the model --
frame normalisation (slowfast/datasets/utils.py:290-307), the log-power STFT of the 24 kHz audio (data/preprocess.py:276-290,
offline with librosa there), the T spectrogram windows around the sampled frames (ego4d_avgaze_forecast.py:214-219) and
the Gaussian gaze heat maps (ego4d_avgaze_forecast.py:318-326,404-422) -- as HIP kernels, so a batch can be assembled
from uint8 frames, a waveform and gaze points without leaving the GPU (the fp32 clip never crosses PCIe)."""
from __future__ import annotations

import ctypes as C

import torch

from . import lib as L


def _s():
    return torch.cuda.current_stream().cuda_stream


def _gpu(*ts):
    for t in ts:
        if not t.is_cuda:
            raise L.CstsError("csts_amd.inputs runs on MI355X only: inputs must be GPU tensors")


def normalize_frames(frames_u8: torch.Tensor, mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225)) -> torch.Tensor:
    """uint8 (B, T, H, W, C) -> fp32 (B, C, T, H, W) = (x/255 - mean)/std."""
    _gpu(frames_u8)
    assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 5
    B, T, H, W, Cc = frames_u8.shape
    x = frames_u8.contiguous()
    out = torch.empty(B, Cc, T, H, W, dtype=torch.float32, device=x.device)
    f3 = C.c_float * 3
    L.check(L.load().csts_frames_normalize(x.data_ptr(), out.data_ptr(), B, T * H * W, Cc, f3(*mean), f3(*std), _s()),
            "csts_frames_normalize")
    return out


def stft_logpower(wav: torch.Tensor, n_fft: int = 511, hop: int = 120, win: int = 240, eps: float = 1e-6) -> torch.Tensor:
    """fp32 waveform (B, n) -> log(|STFT|^2 + eps), (B, n_fft//2 + 1, frames) with librosa.stft semantics."""
    _gpu(wav)
    w = wav.contiguous().float()
    B, n = w.shape
    lib = L.load()
    nfr = lib.csts_stft_frames(n, n_fft, hop)
    spec = torch.empty(B, n_fft // 2 + 1, nfr, dtype=torch.float32, device=w.device)
    L.check(lib.csts_stft_logpower(w.data_ptr(), spec.data_ptr(), B, n, n_fft, hop, win, eps, _s()), "csts_stft_logpower")
    return spec


AUDIO_RATE = 24000          # the rate the model's spectrogram is defined at (data/preprocess.py::extract_audio, -ar 24000)
_RULES, _TABLES = {}, {}    # (rate, target, zeros, beta) -> host rule; (..., device) -> fp32 device table


def check_sample_rate(rate, what: str = "sample_rate") -> int:
    """A sample rate is a positive integer (int or numpy integer; no bool, no float): ValueError otherwise."""
    import numbers
    if isinstance(rate, bool) or not isinstance(rate, numbers.Integral) or int(rate) <= 0:
        raise ValueError(f"{what} must be a positive integer number of samples per second, got {rate!r}")
    return int(rate)


def resample_lds_floats(up: int, down: int, half: int) -> int:
    """The LDS floats csts_resample_wav needs (include/csts_hip.h): the phase-major filter table and one run's input span."""
    span = ((L.RESAMPLE_RUN - 1) * down + 2 * half) // up + 2
    return up * (((2 * half + up) // up) | 1) + span + span // 32 + 1


def resample_rule(sample_rate, target_rate=AUDIO_RATE, zeros: int = 10, beta: float = 5.0):
    """The host side of resample_audio, fp64, cached: (h float64 (2 * half + 1,), up, down, half) with up / down = target_rate /
    sample_rate reduced by their gcd, half = zeros * max(up, down) and h the windowed sinc scipy.signal.resample_poly designs,
    h = sinc(k / mx) / mx * kaiser(2 half + 1, beta), k = -half .. half, scaled to sum to up.  A ratio whose table does not fit
    csts_resample_wav is a ValueError naming the reduced ratio."""
    import math
    import numpy as np
    sample_rate, target_rate = check_sample_rate(sample_rate), check_sample_rate(target_rate, "target_rate")
    zeros, beta = int(zeros), float(beta)
    if zeros < 1 or not beta >= 0.0:
        raise ValueError(f"zeros must be positive and beta non-negative, got {zeros} and {beta}")
    key = (sample_rate, target_rate, zeros, beta)
    if key not in _RULES:
        g = math.gcd(sample_rate, target_rate)
        up, down = target_rate // g, sample_rate // g
        mx = max(up, down)
        half = zeros * mx
        if mx > L.RESAMPLE_MAX_RATIO or half > L.RESAMPLE_MAX_RATIO or resample_lds_floats(up, down, half) > L.RESAMPLE_MAX_LDS_FLOATS:
            raise ValueError(f"{sample_rate} Hz -> {target_rate} Hz reduces to the ratio {up}/{down}: its filter of {2 * half + 1} taps "
                             "is beyond the table the resampling kernel supports (there is no fallback)")
        k = np.arange(-half, half + 1, dtype=np.float64)
        h = np.sinc(k / mx) / mx * np.kaiser(2 * half + 1, beta)
        h = h / h.sum() * up
        h.setflags(write=False)
        _RULES[key] = (h, up, down, half)
    return _RULES[key]


def resample_filter(sample_rate, target_rate=AUDIO_RATE, zeros: int = 10, beta: float = 5.0, device=None):
    """(taps fp32 (2 * half + 1,) on `device` (default: the current GPU), up, down, half): resample_rule's table as
    csts_resample_wav reads it, cached per (sample_rate, target_rate, zeros, beta, device)."""
    h, up, down, half = resample_rule(sample_rate, target_rate, zeros, beta)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise L.CstsError("csts_amd.inputs runs on MI355X only: the filter table lives on a GPU device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(sample_rate), int(target_rate), int(zeros), float(beta), device)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(h.astype("float32")).to(device)
    return _TABLES[key], up, down, half


def resample_audio(wav: torch.Tensor, sample_rate, target_rate=AUDIO_RATE, zeros: int = 10, beta: float = 5.0) -> torch.Tensor:
    """A waveform at any sample rate -> fp32 at target_rate (24 kHz, what stft_logpower expects), on the device in one launch
    (csts_resample_wav): wav (n,), (B, n) or (B, C, n), floating or int16 (scaled by 1 / 32768) -> (n_out,) or (B, n_out),
    n_out = ceil(n * up / down).  The C channels are averaged as the samples are read (ffmpeg's -ac 1) and the mono signal is
    resampled by resample_rule's filter with zero extension at both ends: scipy.signal.resample_poly(x, up, down).
    sample_rate == target_rate with a mono fp32 waveform returns the argument itself and launches nothing."""
    h, up, down, half = resample_rule(sample_rate, target_rate, zeros, beta)
    if not torch.is_tensor(wav) or wav.dim() not in (1, 2, 3) or not (wav.is_floating_point() or wav.dtype == torch.int16):
        raise ValueError("wav must be a floating or int16 tensor (n,), (B, n) or (B, C, n), got "
                         f"{tuple(wav.shape) if torch.is_tensor(wav) else type(wav)} {getattr(wav, 'dtype', '')}")
    if wav.numel() == 0:
        raise ValueError(f"wav holds no sample: {tuple(wav.shape)}")
    _gpu(wav)
    if up == down and wav.dim() < 3 and wav.dtype == torch.float32:
        return wav
    x = wav if wav.dtype in (torch.float32, torch.int16) else wav.float()
    x = (x.reshape(1, 1, -1) if x.dim() == 1 else x.unsqueeze(1) if x.dim() == 2 else x).contiguous()
    B, Cn, n = x.shape
    if B > 65535 or Cn > 64 or n > L.RESAMPLE_MAX_N:
        raise ValueError(f"resample_audio takes B <= 65535 waveforms of C <= 64 channels, got {tuple(wav.shape)}")
    lib = L.load()
    taps = resample_filter(sample_rate, target_rate, zeros, beta, x.device)[0]
    n_out = lib.csts_resample_len(n, up, down)
    out = torch.empty(B, n_out, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(lib.csts_resample_wav(x.data_ptr(), L.WAV_I16 if x.dtype == torch.int16 else L.WAV_F32, B, Cn, n, taps.data_ptr(), up,
                                      down, half, out.data_ptr(), _s()), "csts_resample_wav")
    return out[0] if wav.dim() == 1 else out


def resample_ready(n_in: int, up: int, down: int, half: int, closed: bool = False) -> int:
    """The outputs of resample_audio's rule that are final after n_in inputs (csts_resample_ready): output m reads the inputs up
    to floor((m down + half) / up), so an open stream has max(0, floor((n_in up - half - 1) / down) + 1) of them; a stream that
    ended at n_in has them all, ceil(n_in up / down)."""
    n_in, up, down, half = int(n_in), int(up), int(down), int(half)
    if closed:
        return -(-n_in * up // down)
    return max(0, (n_in * up - half - 1) // down + 1)


def resample_first_input(m: int, up: int, down: int, half: int) -> int:
    """The first input output m reads (csts_resample_first_input): max(ceil((m down - half) / up), 0)."""
    return max(-(-(int(m) * int(down) - int(half)) // int(up)), 0)


def resample_inputs_for(m_out: int, up: int, down: int, half: int) -> int:
    """The least n_in with resample_ready(n_in) >= m_out: how many source samples an open stream needs before its first m_out
    outputs are final (a window's ready_samples at 24 kHz -> the source samples it waits for).  0 for m_out <= 0."""
    m_out = int(m_out)
    return 0 if m_out <= 0 else ((m_out - 1) * int(down) + int(half)) // int(up) + 1


class StreamResampler:
    """resample_audio on a stream that arrives in pieces: push(piece) returns the 24 kHz samples that piece makes final, close()
    the rest, and torch.cat([*pushes, close()]) equals resample_audio of the whole waveform bit for bit, however it was cut
    (csts_resample_stream runs csts_resample_wav's kernel on the kept tail + the piece, at the stream's positions).

    Pieces are (m,) or (C, m), floating or int16, on the device, m >= 0; the first push fixes `channels` and `dtype`.  The state
    carried between pushes is the tail of the input the unfinished outputs still read, (C, tail) in the input's type with
    tail <= 2 half / up + 2 (42 samples at 48 kHz, 162 at 192 kHz): int16 stays int16 and the downmix happens in the kernel.  A
    push is one torch.cat and one launch, with no host synchronisation.  `consumed` / `produced` count inputs and outputs so far;
    produced == resample_ready(consumed) until close().  sample_rate == target_rate with (m,) fp32 pieces hands the pieces
    through untouched and without delay, as resample_audio returns its argument; any other form at that rate goes through the
    1/1 filter like the offline path."""

    def __init__(self, sample_rate, target_rate=AUDIO_RATE, zeros: int = 10, beta: float = 5.0):
        _, self.up, self.down, self.half = resample_rule(sample_rate, target_rate, zeros, beta)
        self._key = (int(sample_rate), int(target_rate), int(zeros), float(beta))
        self.consumed = self.produced = 0
        self.channels = self.dtype = None
        self.closed = False
        self._mono = self._device = None          # the rank of the pieces, (m,) or (C, m), and their device: the first push's
        self._tail, self._tail_base = None, 0     # (C, tail) of the input and the stream position of its first sample

    def _through(self, wav=None):
        """Pieces pass through untouched: the ratio is 1/1 and they are (m,) fp32."""
        if self.up != self.down:
            return False
        if self.dtype is not None:
            return self._mono and self.dtype == torch.float32
        return wav is not None and wav.dim() == 1 and wav.dtype == torch.float32

    def check(self, wav) -> int:
        """The samples per channel of a piece push() would take; ValueError / CstsError otherwise.  Changes nothing."""
        if self.closed:
            raise ValueError("the resampler is closed: push() after close()")
        if not torch.is_tensor(wav) or wav.dim() not in (1, 2) or not (wav.is_floating_point() or wav.dtype == torch.int16):
            raise ValueError("a piece must be a floating or int16 tensor (m,) or (C, m), got "
                             f"{tuple(wav.shape) if torch.is_tensor(wav) else type(wav)} {getattr(wav, 'dtype', '')}")
        _gpu(wav)
        C = 1 if wav.dim() == 1 else wav.shape[0]
        if C < 1 or C > 64:
            raise ValueError(f"a piece holds 1 <= C <= 64 channels, got {tuple(wav.shape)}")
        if self.dtype is not None and (wav.dtype != self.dtype or C != self.channels or (wav.dim() == 1) != self._mono):
            raise ValueError(f"the stream's pieces are {'(m,)' if self._mono else f'({self.channels}, m)'} {self.dtype} (fixed by "
                             f"the first push), got {tuple(wav.shape)} {wav.dtype}")
        if self.consumed + wav.shape[-1] > L.RESAMPLE_MAX_N:
            raise ValueError(f"a stream holds at most {L.RESAMPLE_MAX_N} samples")
        return int(wav.shape[-1])

    def count(self, m: int, like=None) -> int:
        """How many outputs a push of m more samples would return: host arithmetic, no device work, no state change.  like: the
        piece itself, which a 1/1 stream needs before its first push to tell whether pieces pass through."""
        m = int(m)
        if m < 0:
            raise ValueError(f"a piece holds m >= 0 samples, got {m}")
        if self._through(like):
            return m
        return resample_ready(self.consumed + m, self.up, self.down, self.half) - self.produced

    def _launch(self, buf, n_total, m1):
        out = torch.empty(m1 - self.produced, dtype=torch.float32, device=buf.device)
        if m1 > self.produced:
            taps = resample_filter(*self._key, buf.device)[0]
            with torch.cuda.device(buf.device):
                L.check(L.load().csts_resample_stream(buf.data_ptr(), L.WAV_I16 if buf.dtype == torch.int16 else L.WAV_F32,
                                                      buf.shape[0], buf.shape[1], self._tail_base, n_total, taps.data_ptr(), self.up,
                                                      self.down, self.half, self.produced, m1, out.data_ptr(), _s()),
                        "csts_resample_stream")
        self.produced = m1
        return out

    def push(self, wav: torch.Tensor) -> torch.Tensor:
        """The next piece -> the fp32 (count(m),) outputs it makes final (possibly none)."""
        m = self.check(wav)
        if self.dtype is None:
            self.dtype, self.channels, self._mono = wav.dtype, 1 if wav.dim() == 1 else wav.shape[0], wav.dim() == 1
            self._device = wav.device
        if self._through():
            self.consumed += m
            self.produced += m
            return wav
        x = wav if wav.dtype in (torch.float32, torch.int16) else wav.float()
        x = x.reshape(1, -1) if x.dim() == 1 else x
        buf = torch.cat([self._tail, x], dim=1) if self._tail is not None else torch.cat([x], dim=1)
        self.consumed += m
        out = self._launch(buf, -1, resample_ready(self.consumed, self.up, self.down, self.half))
        keep = max(resample_first_input(self.produced, self.up, self.down, self.half), self._tail_base)
        self._tail, self._tail_base = buf[:, keep - self._tail_base:], keep      # a view: the next push copies it into its buffer
        return out

    def close(self) -> torch.Tensor:
        """End the stream -> the remaining outputs, up to ceil(consumed up / down) (none for a stream that never got a sample)."""
        if self.closed:
            raise ValueError("the resampler is closed already")
        self.closed = True
        if self._tail is None or self._tail.shape[1] == 0:                        # no sample yet, or pieces that pass through
            return torch.empty(0, dtype=torch.float32, device=self._device)
        out = self._launch(self._tail.contiguous(), self.consumed, resample_ready(self.consumed, self.up, self.down, self.half, True))
        self._tail = None
        return out


def audio_windows(spec: torch.Tensor, frames_idx: torch.Tensor, frame_length: float, width: int = 256) -> torch.Tensor:
    """(B, nbins, cols) spectrogram + per-clip frame indices (B, T) -> (B, 1, T, nbins, width) windows centred at
    round(idx / frame_length * cols), clipped to the valid range (ego4d_avgaze_forecast.py:216-219)."""
    _gpu(spec, frames_idx)
    B, nbins, cols = spec.shape
    T = frames_idx.shape[1]
    centers = torch.round(frames_idx.double() / frame_length * cols).to(torch.int32).clamp_(width // 2, cols - 1 - width // 2)
    centers = centers.contiguous()
    out = torch.empty(B, 1, T, nbins, width, dtype=torch.float32, device=spec.device)
    L.check(L.load().csts_audio_windows(spec.contiguous().data_ptr(), centers.data_ptr(), out.data_ptr(), B, T, nbins, cols, width,
                                        _s()), "csts_audio_windows")
    return out


def audio_windows_at(spec: torch.Tensor, centers: torch.Tensor, width: int = 256) -> torch.Tensor:
    """Windows of ONE spectrogram at given centre columns: spec (nbins, cols) or (1, nbins, cols) + centers int (B, T) ->
    (B, 1, T, nbins, width), window (b, t) = spec[:, c - width/2 : c + width/2] (csts_audio_windows).  For clips that are windows
    of one recording and share its spectrogram (infer.plan_video works the centres out); centres are kept inside
    [width/2, cols - 1 - width/2] as audio_windows keeps them."""
    _gpu(spec, centers)
    if spec.dim() == 3 and spec.shape[0] == 1:
        spec = spec[0]
    if spec.dim() != 2 or centers.dim() != 2 or centers.is_floating_point():
        raise ValueError(f"spec must be (nbins, cols) and centers integer (B, T), got {tuple(spec.shape)} and "
                         f"{tuple(centers.shape)} {centers.dtype}")
    nbins, cols = spec.shape
    B, T = centers.shape
    if cols < width + 1:
        raise ValueError(f"the spectrogram has {cols} columns, a window needs {width + 1}")
    c = centers.to(torch.int32).clamp(width // 2, cols - 1 - width // 2).contiguous()
    out = torch.empty(B, 1, T, nbins, width, dtype=torch.float32, device=spec.device)
    # one "clip" of B * T windows: every window reads the same spectrogram
    L.check(L.load().csts_audio_windows(spec.contiguous().float().data_ptr(), c.data_ptr(), out.data_ptr(), 1, B * T, nbins, cols,
                                        width, _s()), "csts_audio_windows")
    return out


def temporal_indices(video_size: int, num_frames: int, sampling_rate: int, clip_idx: int, num_clips: int, *, target_fps=30,
                     fps=30, use_offset: bool = False, u: float = None):
    """The frames of one clip by the reference's temporal rule, decode-everything path (slowfast/datasets/decoder.py:12-68 and
    the tail of decode(), :396-411) -> (start, end, index): index int64 (num_frames,) numpy.

    clip_size = ((sampling_rate + 1) * (num_frames - 1) + 1) / target_fps * fps; delta = max(video_size - clip_size, 0);
    start = delta * clip_idx / num_clips, or with use_offset floor(delta / 2) (num_clips 1) / clip_idx * floor(delta /
    (num_clips - 1)), or u * delta for clip_idx -1 (random sampling: u in [0, 1) is the variate random.uniform consumed);
    end = start + clip_size - 1; index = linspace(start, end, num_frames) clamped to [0, video_size - 1] and truncated.  The
    linspace is torch's, fp32 on the CPU, as in the reference, so fractional positions truncate identically."""
    import math
    video_size, num_frames, clip_idx, num_clips = int(video_size), int(num_frames), int(clip_idx), int(num_clips)
    if video_size < 1 or num_frames < 1 or num_clips < 1:
        raise ValueError(f"video_size, num_frames and num_clips must be positive, got {video_size}, {num_frames}, {num_clips}")
    clip_size = ((sampling_rate + 1) * (num_frames - 1) + 1) / target_fps * fps
    delta = max(video_size - clip_size, 0)
    if clip_idx == -1:
        if u is None or not 0.0 <= u < 1.0:
            raise ValueError(f"clip_idx -1 (random sampling) needs its variate u in [0, 1), got {u}")
        start = 0 + (delta - 0) * u                     # random.uniform(0, delta)
    elif use_offset:
        start = math.floor(delta / 2) if num_clips == 1 else clip_idx * math.floor(delta / (num_clips - 1))
    else:
        start = delta * clip_idx / num_clips
    end = start + clip_size - 1
    index = torch.clamp(torch.linspace(start, end, num_frames), 0, video_size - 1).long()
    return start, end, index.numpy()


def gaze_heatmaps(labels: torch.Tensor, H: int = 64, W: int = 64, ksize: int = 19) -> torch.Tensor:
    """labels (B, T, >=2) with x, y in [0, 1] -> (B, T, H, W) maps summing to 1 per frame."""
    _gpu(labels)
    lab = labels.contiguous().float()
    B, T, S = lab.shape
    out = torch.empty(B, T, H, W, dtype=torch.float32, device=lab.device)
    L.check(L.load().csts_gaze_heatmaps(lab.data_ptr(), S, out.data_ptr(), B * T, H, W, ksize, _s()), "csts_gaze_heatmaps")
    return out


PIXEL_FORMATS = ("rgb24", "nv12", "i420")     # packed RGB, and the two 4:2:0 layouts of include/csts_hip.h
YUV_MATRICES = ("bt601", "bt709")
# {CY, CRV, CGU, CGV, CBU} = round(c * 2^20) of (matrix, full_range): the tables of include/csts_hip.h, restated
YUV_TABLES = {("bt601", False): (1220945, 1673555, -410793, -852458, 2115221),
              ("bt601", True): (1048576, 1470104, -360853, -748826, 1858077),
              ("bt709", False): (1220945, 1879825, -223607, -558796, 2215014),
              ("bt709", True): (1048576, 1651297, -196424, -490864, 1945738)}


def yuv_frame_shape(H: int, W: int):
    """The shape of one 4:2:0 frame of H x W pixels (H, W even): (H * 3 // 2, W) bytes, the Y plane then the chroma."""
    H, W = int(H), int(W)
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"4:2:0 frames need even H, W >= 2, got {H} x {W}")
    return H * 3 // 2, W


def check_pixel_format(pixel_format, matrix="bt601", full_range=False):
    """(layout, matrix, full_range) as the C ABI takes them; layout 0 for rgb24.  ValueError for an unknown format or matrix."""
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError(f"pixel_format must be one of {PIXEL_FORMATS}, got {pixel_format!r}")
    if matrix not in YUV_MATRICES:
        raise ValueError(f"matrix must be one of {YUV_MATRICES}, got {matrix!r}")
    return PIXEL_FORMATS.index(pixel_format), YUV_MATRICES.index(matrix), int(bool(full_range))


def _yuv_hw(shape, pixel_format, what="frames"):
    """H, W of 4:2:0 pictures whose last two dimensions are (H * 3 / 2, W): ValueError for rows no multiple of 3, odd H or W,
    or a trailing dimension of 3 (packed RGB passed as 4:2:0)."""
    if len(shape) < 2:
        raise ValueError(f"{what} in {pixel_format} must be uint8 (..., H * 3 / 2, W), got {tuple(shape)}")
    rows, W = int(shape[-2]), int(shape[-1])
    if W == 3 and len(shape) >= 3:
        raise ValueError(f"{what} of shape {tuple(shape)} look like packed RGB (..., H, W, 3), not {pixel_format}: pass "
                         "pixel_format='rgb24'")
    if rows < 3 or rows % 3:
        raise ValueError(f"{what} in {pixel_format} hold H * 3 / 2 rows per picture: {rows} is not a multiple of 3")
    H = rows // 3 * 2
    if W < 2 or W % 2 or H % 2:
        raise ValueError(f"{what} in {pixel_format} need even H and W, got H {H}, W {W}")
    return H, W


YUV_MAX_WS = 32768      # CSTS_YUV_MAX_WS of include/csts_hip.h: the widest surface row the *_win entry points take


def check_window(shape, pixel_format, window, what="frames"):
    """The window (top, left, H, W) of 4:2:0 surfaces of `shape` (..., Hs * 3 / 2, Ws), checked: -> (top, left, H, W) as ints,
    or None for window None (the whole surface).  The picture is the H x W pixels whose first is luma (top, left) of the surface
    ("Decoder surfaces", include/csts_hip.h).  ValueError, naming the value: a window given with rgb24, not four integers, an odd
    or negative value, H or W below 2, top + H > Hs, left + W > Ws, Ws > YUV_MAX_WS."""
    if window is None:
        return None
    top, left, H, W = window_values(pixel_format, window)
    Hs, Ws = _yuv_hw(shape, pixel_format, what)
    if top + H > Hs:
        raise ValueError(f"window top {top} + H {H} = {top + H} exceeds the surface height {Hs}")
    if left + W > Ws:
        raise ValueError(f"window left {left} + W {W} = {left + W} exceeds the surface width {Ws}")
    if Ws > YUV_MAX_WS:
        raise ValueError(f"a windowed surface is at most {YUV_MAX_WS} bytes wide, got Ws {Ws}")
    return top, left, H, W


def window_values(pixel_format, window):
    """The rules of check_window that need no surface: -> (top, left, H, W) as ints."""
    if check_pixel_format(pixel_format)[0] == 0:
        raise ValueError(f"window {window!r} is given with pixel_format 'rgb24': a window selects the picture inside a 4:2:0 "
                         "surface ('nv12' | 'i420')")
    try:
        vals = [int(v) for v in window]
        exact = all(v == w for v, w in zip(vals, window))
    except (TypeError, ValueError):
        vals, exact = [], False
    if len(vals) != 4 or not exact:
        raise ValueError(f"window must be four integers (top, left, H, W), got {window!r}")
    top, left, H, W = vals
    for name, v in (("top", top), ("left", left), ("H", H), ("W", W)):
        if v < 0:
            raise ValueError(f"window {name} {v} is negative (window {tuple(vals)})")
        if v % 2:
            raise ValueError(f"window {name} {v} is odd: 4:2:0 windows start and end on a chroma sample (window {tuple(vals)})")
    if H < 2 or W < 2:
        raise ValueError(f"window H {H}, W {W} must be at least 2")
    return top, left, H, W


def _yuv_geom(shape, pixel_format, window, what="frames"):
    """H, W of the picture and the surface arguments of a *_win entry point: (H, W, None) for a tight call -- no window, or the
    window that is the whole surface: today's call -- else (H, W, (Hs, Ws, top, left))."""
    Hs, Ws = _yuv_hw(shape, pixel_format, what)
    win = check_window(shape, pixel_format, window, what)
    if win is None or win == (0, 0, Hs, Ws):
        return Hs, Ws, None
    return win[2], win[3], (Hs, Ws, win[0], win[1])


def window_size(shape, pixel_format, window, what="frames"):
    """H, W of the picture a call with `window` sees in 4:2:0 surfaces of `shape`."""
    return _yuv_geom(shape, pixel_format, window, what)[:2]


def no_window(window, who):
    """The refusal of the callers that take tight pictures only."""
    if window is not None:
        raise ValueError(f"{who} takes tight 4:2:0 pictures only, no window: repack the surface first (inputs.yuv_window)")


def yuv_window(frames, pixel_format: str, window):
    """The repack: the tight 4:2:0 pictures (..., H * 3 / 2, W) of the window (top, left, H, W) of surfaces (..., Hs * 3 / 2, Ws),
    by plain slicing (a torch tensor or a numpy array in, the same kind out, a new contiguous one).  The oracle of every
    window= keyword: f(surface, ..., window=w) == f(yuv_window(surface, pixel_format, w), ...), bit for bit.  window None
    returns the surfaces themselves."""
    win = check_window(frames.shape, pixel_format, window)
    if win is None:
        return frames
    top, left, H, W = win
    Hs, Ws = _yuv_hw(frames.shape, pixel_format)
    lead = tuple(frames.shape[:-2])
    cat = torch.cat if torch.is_tensor(frames) else __import__("numpy").concatenate
    luma = frames[..., top:top + H, left:left + W]
    if pixel_format == "nv12":
        chroma = frames[..., Hs + top // 2:Hs + (top + H) // 2, left:left + W]
        return cat([luma, chroma], -2)
    planes = frames[..., Hs:, :].reshape(lead + (2, Hs // 2, Ws // 2))
    planes = planes[..., top // 2:(top + H) // 2, left // 2:(left + W) // 2]
    return cat([luma, planes.reshape(lead + (H // 2, W))], -2)


def yuv_to_rgb(frames_yuv: torch.Tensor, pixel_format: str, matrix: str = "bt601", full_range: bool = False,
               out: torch.Tensor = None, *, window=None) -> torch.Tensor:
    """4:2:0 pictures uint8 (..., H * 3 / 2, W) in `pixel_format` ("nv12" | "i420") -> packed RGB uint8 (..., H, W, 3) by the
    integer rule of include/csts_hip.h (nearest chroma, `matrix` "bt601" | "bt709", limited range unless full_range), one
    streaming launch (csts_yuv_to_rgb).  The input may start at any byte.  out: a contiguous uint8 (..., H, W, 3) GPU tensor to
    write into, at any byte as well (a slice of a larger tensor); it must not share memory with the input.  window (top, left,
    H, W): the frames are surfaces (..., Hs * 3 / 2, Ws) and the pictures their windows (check_window), read in place
    (csts_yuv_to_rgb_win); the result is the (..., H, W, 3) of the window."""
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    if layout == 0:
        raise ValueError("yuv_to_rgb converts 'nv12' or 'i420' pictures; rgb24 needs no conversion")
    if not torch.is_tensor(frames_yuv) or frames_yuv.dtype != torch.uint8:
        raise ValueError(f"frames must be a uint8 tensor (..., H * 3 / 2, W), got {getattr(frames_yuv, 'dtype', type(frames_yuv))}")
    H, W, surf = _yuv_geom(frames_yuv.shape, pixel_format, window)
    lead = tuple(frames_yuv.shape[:-2])
    N = 1
    for d in lead:
        N *= int(d)
    if N < 1:
        raise ValueError(f"frames hold no picture: {tuple(frames_yuv.shape)}")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != lead + (H, W, 3) or
                            not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 {lead + (H, W, 3)} tensor")
    _gpu(frames_yuv)
    x = frames_yuv.contiguous()
    if out is None:
        out = torch.empty(lead + (H, W, 3), dtype=torch.uint8, device=x.device)
    else:
        _gpu(out)
        a, b = x.data_ptr(), out.data_ptr()
        if out.device != x.device or (a < b + out.numel() and b < a + x.numel()):
            raise ValueError("out must be on the frames' device and must not share memory with them")
    with torch.cuda.device(x.device):
        if surf:
            L.check(L.load().csts_yuv_to_rgb_win(x.data_ptr(), out.data_ptr(), N, H, W, *surf, layout, mat, fr, _s()),
                    "csts_yuv_to_rgb_win")
        else:
            L.check(L.load().csts_yuv_to_rgb(x.data_ptr(), out.data_ptr(), N, H, W, layout, mat, fr, _s()), "csts_yuv_to_rgb")
    return out


def yuv_to_rgb_host(frames_yuv, pixel_format: str, matrix: str = "bt601", full_range: bool = False, *, window=None):
    """yuv_to_rgb on the CPU (csts_yuv_to_rgb_host, the same pixel function): numpy uint8 (..., H * 3 / 2, W) -> (..., H, W, 3);
    window as yuv_to_rgb takes it (csts_yuv_to_rgb_win_host)."""
    import numpy as np
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    if layout == 0:
        raise ValueError("yuv_to_rgb_host converts 'nv12' or 'i420' pictures; rgb24 needs no conversion")
    x = np.ascontiguousarray(frames_yuv)
    if x.dtype != np.uint8:
        raise ValueError(f"frames must be uint8, got {x.dtype}")
    H, W, surf = _yuv_geom(x.shape, pixel_format, window)
    lead = tuple(x.shape[:-2])
    N = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if N < 1:
        raise ValueError(f"frames hold no picture: {x.shape}")
    out = np.empty(lead + (H, W, 3), dtype=np.uint8)
    if surf:
        L.check(L.load().csts_yuv_to_rgb_win_host(x.ctypes.data, out.ctypes.data, N, H, W, *surf, layout, mat, fr),
                "csts_yuv_to_rgb_win_host")
    else:
        L.check(L.load().csts_yuv_to_rgb_host(x.ctypes.data, out.ctypes.data, N, H, W, layout, mat, fr), "csts_yuv_to_rgb_host")
    return out


# {YR, YG, YB, UR, UG, UB, VR, VG, VB} = round(c * 2^20) of (matrix, full_range): the inverse tables of include/csts_hip.h, restated
RGB_TABLES = {("bt601", False): (269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897),
              ("bt601", True): (313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262),
              ("bt709", False): (191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230),
              ("bt709", True): (222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074)}


def _rgb_hw(shape, what="frames"):
    """lead, H, W of packed RGB pictures (..., H, W, 3) that are to become 4:2:0 ones: ValueError for another shape, odd H or W."""
    if len(shape) < 3 or int(shape[-1]) != 3:
        raise ValueError(f"{what} must be uint8 (..., H, W, 3) packed RGB, got {tuple(shape)}")
    H, W = int(shape[-3]), int(shape[-2])
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"4:2:0 pictures need even H and W, got H {H}, W {W}")
    return tuple(int(d) for d in shape[:-3]), H, W


def rgb_to_yuv(frames_u8: torch.Tensor, pixel_format: str, matrix: str = "bt601", full_range: bool = False,
               out: torch.Tensor = None, *, window=None) -> torch.Tensor:
    """Packed RGB uint8 (..., H, W, 3), H and W even -> 4:2:0 pictures uint8 (..., H * 3 / 2, W) in `pixel_format` ("nv12" |
    "i420") by the inverse integer rule of include/csts_hip.h (luma per pixel, chroma from the sums of each 2 x 2 block; `matrix`
    "bt601" | "bt709", limited range unless full_range), one streaming launch (csts_rgb_to_yuv).  The input may start at any
    byte.  out: a contiguous uint8 (..., H * 3 / 2, W) GPU tensor to write into, at any byte as well; it must not share memory
    with the input.  It writes tight pictures only: a window (writing into a decoder surface) is refused."""
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    if layout == 0:
        raise ValueError("rgb_to_yuv writes 'nv12' or 'i420' pictures; rgb24 needs no conversion")
    if window is not None:
        raise ValueError("rgb_to_yuv writes tight 4:2:0 pictures only: writing the window of a surface is not supported")
    if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8:
        raise ValueError(f"frames must be a uint8 tensor (..., H, W, 3), got {getattr(frames_u8, 'dtype', type(frames_u8))}")
    lead, H, W = _rgb_hw(frames_u8.shape)
    N = 1
    for d in lead:
        N *= d
    if N < 1:
        raise ValueError(f"frames hold no picture: {tuple(frames_u8.shape)}")
    shape = lead + (H * 3 // 2, W)
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != shape or
                            not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 {shape} tensor")
    _gpu(frames_u8)
    x = frames_u8.contiguous()
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    else:
        _gpu(out)
        a, b = x.data_ptr(), out.data_ptr()
        if out.device != x.device or (a < b + out.numel() and b < a + x.numel()):
            raise ValueError("out must be on the frames' device and must not share memory with them")
    with torch.cuda.device(x.device):
        L.check(L.load().csts_rgb_to_yuv(x.data_ptr(), out.data_ptr(), N, H, W, layout, mat, fr, _s()), "csts_rgb_to_yuv")
    return out


def rgb_to_yuv_host(frames_u8, pixel_format: str, matrix: str = "bt601", full_range: bool = False):
    """rgb_to_yuv on the CPU (csts_rgb_to_yuv_host, the same functions): numpy uint8 (..., H, W, 3) -> (..., H * 3 / 2, W)."""
    import numpy as np
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    if layout == 0:
        raise ValueError("rgb_to_yuv_host writes 'nv12' or 'i420' pictures; rgb24 needs no conversion")
    x = np.ascontiguousarray(frames_u8)
    if x.dtype != np.uint8:
        raise ValueError(f"frames must be uint8, got {x.dtype}")
    lead, H, W = _rgb_hw(x.shape)
    N = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if N < 1:
        raise ValueError(f"frames hold no picture: {x.shape}")
    out = np.empty(lead + (H * 3 // 2, W), dtype=np.uint8)
    L.check(L.load().csts_rgb_to_yuv_host(x.ctypes.data, out.ctypes.data, N, H, W, layout, mat, fr), "csts_rgb_to_yuv_host")
    return out


def spatial_sampling(frames_u8: torch.Tensor, labels: torch.Tensor, crop_size: int, *, train: bool, min_scale: int = 0,
                     max_scale: int = 0, spatial_idx: int = 1, random_flip: bool = True, inverse_uniform: bool = False,
                     mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225), generator=None, return_params: bool = False,
                     key: torch.Tensor = None, pixel_format: str = "rgb24", matrix: str = "bt601", full_range: bool = False,
                     window=None):
    """slowfast/datasets/utils.py::spatial_sampling(..., gaze_loc=labels) on the device, fused with frame normalisation.

    frames_u8 uint8 (B, T, H, W, 3), labels (B, T, L >= 2) with x, y in columns 0, 1 -> video fp32 (B, 3, T, S, S) and the
    transformed labels fp64 (B, T, L) [and the int32 params (B, 5) = new h, new w, y0, x0, flip].  train=True: short-side
    jitter in [min_scale, max_scale] (DATA.TRAIN_JITTER_SCALES), gaze-aware random crop, flip with probability 0.5
    (DATA.RANDOM_FLIP); the clip variates come from a 64-bit key drawn once per call from `generator` (torch's default
    device generator when None), so the call needs no host sync, can be captured in a graph and follows torch.manual_seed.
    train=False: short side resized to crop_size and the uniform crop `spatial_idx` (0, 1, 2); no draw.  key: an int64 (1,)
    device tensor to use instead of the draw (the kernel reads it when it runs).  include/csts_hip.h states the rule.
    pixel_format "nv12" | "i420": frames_u8 is uint8 (B, T, H * 3 / 2, W), 4:2:0 pictures sampled in place (spatial_sample);
    window (top, left, H, W): the pictures are the windows of surfaces (B, T, Hs * 3 / 2, Ws) (check_window), and the rule runs
    on the window's H x W."""
    yuv = check_pixel_format(pixel_format, matrix, full_range)[0] != 0
    if yuv:
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
            raise ValueError(f"{pixel_format} frames must be uint8 (B, T, H * 3 / 2, W), got {tuple(frames_u8.shape)} "
                             f"{frames_u8.dtype}")
        (B, T), (H, W) = frames_u8.shape[:2], window_size(frames_u8.shape, pixel_format, window)
    else:
        check_window(frames_u8.shape, pixel_format, window)
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 5 or frames_u8.shape[-1] != 3:
            raise ValueError(f"frames must be uint8 (B, T, H, W, 3), got {tuple(frames_u8.shape)} {frames_u8.dtype}")
        B, T, H, W, _ = frames_u8.shape
    if labels.dim() != 3 or tuple(labels.shape[:2]) != (B, T) or labels.shape[2] < 2 or not labels.is_floating_point():
        raise ValueError(f"labels must be floating (B, T, L >= 2) = ({B}, {T}, L), got {tuple(labels.shape)} {labels.dtype}")
    S = int(crop_size)
    if not 1 <= T <= 64:
        raise ValueError(f"spatial sampling takes 1 <= T <= 64 frames per clip, got {T}")
    if S < 1:
        raise ValueError(f"crop_size must be positive, got {S}")
    if train:
        min_scale, max_scale = int(min_scale), int(max_scale)
        if min_scale < S:
            raise ValueError(f"the short side would end up below the crop: min_scale {min_scale} < crop_size {S}")
        if max_scale < min_scale:
            raise ValueError(f"max_scale {max_scale} < min_scale {min_scale}")
        idx = -1
    else:
        idx = int(spatial_idx)
        if idx not in (0, 1, 2):
            raise ValueError(f"spatial_idx must be 0, 1 or 2 in test mode, got {spatial_idx}")
    _gpu(frames_u8, labels)
    x = frames_u8.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    lab = labels.to(torch.float64).contiguous()
    ncol = lab.shape[2]
    dev = x.device
    lib = L.load()
    if not train:
        key = None
    elif key is None:
        key = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=dev, generator=generator)
    elif key.dtype != torch.int64 or key.numel() != 1 or key.device != dev:
        raise ValueError("key must be an int64 tensor of one element on the frames' device")
    params = torch.empty(B, 5, dtype=torch.int32, device=dev)
    new_labels = torch.empty_like(lab)
    L.check(lib.csts_spatial_params(key.data_ptr() if key is not None else None, lab.data_ptr(), B, T, ncol, H, W, S, min_scale,
                                     max_scale, idx, int(bool(random_flip)), int(bool(inverse_uniform)), params.data_ptr(),
                                     new_labels.data_ptr(), _s()), "csts_spatial_params")
    video = spatial_sample(x, params, S, mean=mean, std=std, pixel_format=pixel_format, matrix=matrix, full_range=full_range,
                           window=window)
    return (video, new_labels, params) if return_params else (video, new_labels)


def spatial_sample(frames_u8: torch.Tensor, params: torch.Tensor, crop_size: int, mean=(0.45, 0.45, 0.45),
                   std=(0.225, 0.225, 0.225), *, pixel_format: str = "rgb24", matrix: str = "bt601",
                   full_range: bool = False, window=None) -> torch.Tensor:
    """The pixel pass of spatial_sampling alone: uint8 (B, T, H, W, 3) + int32 params (B, 5) = new h, new w, y0, x0, flip ->
    fp32 (B, 3, T, S, S) = normalised bilinear resize (F.interpolate, align_corners=False) + crop + horizontal flip.
    pixel_format "nv12" | "i420": frames_u8 is uint8 (B, T, H * 3 / 2, W), 4:2:0 pictures read in place
    (csts_spatial_sample_yuv); the result is, bit for bit, spatial_sample(yuv_to_rgb(frames, ...), params, S).  window (top,
    left, H, W): the pictures are the windows of surfaces (B, T, Hs * 3 / 2, Ws), read in place (csts_spatial_sample_yuv_win)."""
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    surf = None
    if layout:
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
            raise ValueError(f"{pixel_format} frames must be uint8 (B, T, H * 3 / 2, W), got {tuple(frames_u8.shape)} "
                             f"{frames_u8.dtype}")
        (B, T), (H, W, surf) = frames_u8.shape[:2], _yuv_geom(frames_u8.shape, pixel_format, window)
    else:
        check_window(frames_u8.shape, pixel_format, window)
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 5 or frames_u8.shape[-1] != 3:
            raise ValueError(f"frames must be uint8 (B, T, H, W, 3), got {tuple(frames_u8.shape)} {frames_u8.dtype}")
        B, T, H, W, _ = frames_u8.shape
    if params.dtype != torch.int32 or tuple(params.shape) != (B, 5):
        raise ValueError(f"params must be int32 ({B}, 5), got {tuple(params.shape)} {params.dtype}")
    _gpu(frames_u8, params)
    x = frames_u8.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    S = int(crop_size)
    out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=x.device)
    f3 = C.c_float * 3
    par = params.contiguous()
    if surf:
        L.check(L.load().csts_spatial_sample_yuv_win(x.data_ptr(), par.data_ptr(), out.data_ptr(), B, T, H, W, *surf, S, f3(*mean),
                                                     f3(*std), layout, mat, fr, _s()), "csts_spatial_sample_yuv_win")
        return out
    if layout:
        L.check(L.load().csts_spatial_sample_yuv(x.data_ptr(), par.data_ptr(), out.data_ptr(), B, T, H, W, S, f3(*mean), f3(*std),
                                                 layout, mat, fr, _s()), "csts_spatial_sample_yuv")
        return out
    L.check(L.load().csts_spatial_sample(x.data_ptr(), par.data_ptr(), out.data_ptr(), B, T, H, W, S, f3(*mean), f3(*std), _s()),
            "csts_spatial_sample")
    return out


def clip_sample(video_u8: torch.Tensor, frames_idx: torch.Tensor, params: torch.Tensor, crop_size: int,
                mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225), *, pixel_format: str = "rgb24", matrix: str = "bt601",
                full_range: bool = False, window=None) -> torch.Tensor:
    """spatial_sample of clips that are windows of ONE resident video, without gathering them first: video uint8 (N, H, W, 3),
    frames_idx int32 (B, T) frame numbers (clamped to [0, N - 1] on the device, as the reference's temporal_sampling clamps),
    params int32 (B, 5) -> fp32 (B, 3, T, S, S), bit for bit spatial_sample(video[frames_idx], params, S).  The table is read
    by the kernel when it runs: no host sync, graph-capturable (csts_clip_sample).  pixel_format "nv12" | "i420": the video is
    uint8 (N, H * 3 / 2, W), 4:2:0 pictures read in place (csts_clip_sample_yuv), bit for bit clip_sample of yuv_to_rgb(video).
    window (top, left, H, W): the video holds surfaces (N, Hs * 3 / 2, Ws) and its pictures are their windows
    (csts_clip_sample_yuv_win)."""
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    surf = None
    if layout:
        if video_u8.dtype != torch.uint8 or video_u8.dim() != 3 or video_u8.shape[0] < 1:
            raise ValueError(f"{pixel_format} video must be uint8 (N >= 1, H * 3 / 2, W), got {tuple(video_u8.shape)} "
                             f"{video_u8.dtype}")
        N, (H, W, surf) = video_u8.shape[0], _yuv_geom(video_u8.shape, pixel_format, window, "video")
    else:
        check_window(video_u8.shape, pixel_format, window)
        if video_u8.dtype != torch.uint8 or video_u8.dim() != 4 or video_u8.shape[-1] != 3 or video_u8.shape[0] < 1:
            raise ValueError(f"video must be uint8 (N >= 1, H, W, 3), got {tuple(video_u8.shape)} {video_u8.dtype}")
        N, H, W, _ = video_u8.shape
    if frames_idx.dtype != torch.int32 or frames_idx.dim() != 2:
        raise ValueError(f"frames_idx must be int32 (B, T), got {tuple(frames_idx.shape)} {frames_idx.dtype}")
    B, T = frames_idx.shape
    if not 1 <= T <= 64 or B < 1:
        raise ValueError(f"clip sampling takes B >= 1 clips of 1 <= T <= 64 frames, got B {B}, T {T}")
    if params.dtype != torch.int32 or tuple(params.shape) != (B, 5):
        raise ValueError(f"params must be int32 ({B}, 5), got {tuple(params.shape)} {params.dtype}")
    S = int(crop_size)
    if S < 1:
        raise ValueError(f"crop_size must be positive, got {S}")
    _gpu(video_u8, frames_idx, params)
    x = video_u8.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=x.device)
    f3 = C.c_float * 3
    idx, par = frames_idx.contiguous(), params.contiguous()
    if surf:
        L.check(L.load().csts_clip_sample_yuv_win(x.data_ptr(), N, idx.data_ptr(), par.data_ptr(), out.data_ptr(), B, T, H, W, *surf,
                                                  S, f3(*mean), f3(*std), layout, mat, fr, _s()), "csts_clip_sample_yuv_win")
        return out
    if layout:
        L.check(L.load().csts_clip_sample_yuv(x.data_ptr(), N, idx.data_ptr(), par.data_ptr(), out.data_ptr(), B, T, H, W, S,
                                              f3(*mean), f3(*std), layout, mat, fr, _s()), "csts_clip_sample_yuv")
        return out
    L.check(L.load().csts_clip_sample(x.data_ptr(), N, idx.data_ptr(), par.data_ptr(), out.data_ptr(), B, T, H, W, S, f3(*mean),
                                      f3(*std), _s()), "csts_clip_sample")
    return out


STFT_N_FFT, STFT_HOP, STFT_WIN, STFT_EPS = 511, 120, 240, 1e-6     # stft_logpower's defaults: the model's spectrogram


def stream_stft(buf: torch.Tensor, s_base: int, f0: int, f1: int, ring: torch.Tensor, n_total: int = -1, n_fft: int = STFT_N_FFT,
                hop: int = STFT_HOP, win: int = STFT_WIN, eps: float = STFT_EPS) -> torch.Tensor:
    """Columns [f0, f1) of stft_logpower's spectrogram of an endless signal, written into a spectrogram ring (csts_stream_stft):
    buf fp32 (m,) holds the samples [s_base, s_base + m) of the signal, ring fp32 (n_fft // 2 + 1, ring_cols) receives column f at
    ring[:, f % ring_cols].  Column f reads the samples [f * hop + (n_fft - win) // 2 - n_fft // 2, + win) -- [120 f - 120,
    120 f + 120) with the defaults; samples before 0 are zero and, with n_total >= 0 (the signal ended after n_total samples), so
    are those at or past n_total, as at the two ends of an offline waveform.  A column that needs any other sample the buffer
    does not hold, or more than ring_cols columns at once, is a ValueError.  Column f equals stft_logpower(whole signal)[:, f]
    bit for bit (one device function computes both).  Returns the ring."""
    _gpu(buf, ring)
    s_base, f0, f1, n_total = int(s_base), int(f0), int(f1), int(n_total)
    if buf.dtype != torch.float32 or buf.dim() != 1 or not buf.is_contiguous():
        raise ValueError(f"buf must be a contiguous fp32 (m,) waveform, got {tuple(buf.shape)} {buf.dtype}")
    nbins = n_fft // 2 + 1
    if ring.dtype != torch.float32 or ring.dim() != 2 or ring.shape[0] != nbins or not ring.is_contiguous():
        raise ValueError(f"the ring must be contiguous fp32 ({nbins}, ring_cols), got {tuple(ring.shape)} {ring.dtype}")
    m, ring_cols = buf.numel(), ring.shape[1]
    if s_base < 0 or f0 < 0 or f1 <= f0 or f1 - f0 > ring_cols:
        raise ValueError(f"columns [{f0}, {f1}) must be non-empty and at most one turn of the ring ({ring_cols} columns); s_base "
                         f"{s_base} >= 0")
    if n_total >= 0 and n_total > s_base + m:
        raise ValueError(f"n_total {n_total} lies past the {s_base + m} samples pushed")
    first = max(f0 * hop + (n_fft - win) // 2 - n_fft // 2, 0)
    last = (f1 - 1) * hop + (n_fft - win) // 2 - n_fft // 2 + win
    if n_total >= 0:
        last = min(last, n_total)
    if last > first and (first < s_base or last > s_base + m):
        raise ValueError(f"columns [{f0}, {f1}) read the samples [{first}, {last}), the buffer holds [{s_base}, {s_base + m})")
    with torch.cuda.device(ring.device):
        L.check(L.load().csts_stream_stft(buf.data_ptr() if m else None, s_base, m, n_total, f0, f1, ring.data_ptr(), ring_cols,
                                          n_fft, hop, win, eps, _s()), "csts_stream_stft")
    return ring


def stream_audio_windows(ring: torch.Tensor, newest: int, centers: torch.Tensor, centers_host, width: int = 256) -> torch.Tensor:
    """audio_windows_at on a spectrogram ring (csts_stream_audio_windows): ring fp32 (nbins, ring_cols) holds column f of an endless
    spectrogram at ring[:, f % ring_cols] (stream_stft), newest is the last column written, centers int64 (B, T) on the device are
    GLOBAL centre columns -> (B, 1, T, nbins, width), window (b, t) = columns [c - width/2, c + width/2) read across the wrap.
    Nothing is clamped: centers_host, the same table on the host (anything numpy.asarray takes), is checked first and a window
    that is not wholly inside the live span [max(newest - ring_cols + 1, 0), newest] is a ValueError; the device applies the same
    test when the kernel runs and gives such a window NaN, so a replayed launch stays safe."""
    import numpy as np
    _gpu(ring, centers)
    if ring.dtype != torch.float32 or ring.dim() != 2 or not ring.is_contiguous():
        raise ValueError(f"the ring must be contiguous fp32 (nbins, ring_cols), got {tuple(ring.shape)} {ring.dtype}")
    if centers.dtype != torch.int64 or centers.dim() != 2:
        raise ValueError(f"centers must be int64 (B, T), got {tuple(centers.shape)} {centers.dtype}")
    nbins, ring_cols = ring.shape
    B, T = centers.shape
    width, newest = int(width), int(newest)
    if width < 2 or width % 2 or width > ring_cols or B < 1 or T < 1 or B * T > 65535:
        raise ValueError(f"bad sizes: width {width} (even, <= ring_cols {ring_cols}), B {B}, T {T} (B * T <= 65535)")
    host = np.asarray(centers_host, dtype=np.int64)
    if host.shape != (B, T):
        raise ValueError(f"the host centre table is {host.shape}, the device one ({B}, {T})")
    oldest = max(newest - ring_cols + 1, 0)
    if int(host.min()) - width // 2 < oldest or int(host.max()) + width // 2 - 1 > newest:
        raise ValueError(f"an audio window reaches outside the ring's live columns [{oldest}, {newest}] ({ring_cols} columns): "
                         f"centres {int(host.min())} .. {int(host.max())}, width {width}")
    out = torch.empty(B, 1, T, nbins, width, dtype=torch.float32, device=ring.device)
    with torch.cuda.device(ring.device):
        L.check(L.load().csts_stream_audio_windows(ring.data_ptr(), ring_cols, newest, centers.contiguous().data_ptr(), out.data_ptr(),
                                                   B, T, nbins, width, _s()), "csts_stream_audio_windows")
    return out


def stream_ingest(chunk_u8: torch.Tensor, pairs: torch.Tensor, params_row: torch.Tensor, ring: torch.Tensor,
                  mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225), *, pixel_format: str = "rgb24", matrix: str = "bt601",
                  full_range: bool = False, window=None) -> torch.Tensor:
    """The used frames of one pushed chunk, sampled once into a ring of normalised crops (csts_stream_ingest): chunk uint8
    (K, H, W, 3), pairs int32 (P, 2) = (frame in chunk, slot) on the device, params_row int32 (5,) = new h, new w, y0, x0, flip
    (one test-mode row for the stream), ring fp32 (R, 3, S, S) -> ring[slot] = clip_sample(chunk, [[frame]], params_row[None],
    S)[0, :, 0], bit for bit.  A chunk frame no pair names is not read, and no other slot is written.  The table is read by the
    kernel when it runs; a pair outside the chunk or the ring writes nothing.  P == 0 launches nothing.  pixel_format "nv12" |
    "i420": the chunk is uint8 (K, H * 3 / 2, W), read in place (csts_stream_ingest_yuv); window (top, left, H, W): the chunk
    holds surfaces (K, Hs * 3 / 2, Ws) and its frames are their windows (csts_stream_ingest_yuv_win).  Returns the ring."""
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    surf = None
    if layout:
        if chunk_u8.dtype != torch.uint8 or chunk_u8.dim() != 3 or chunk_u8.shape[0] < 1:
            raise ValueError(f"{pixel_format} chunk must be uint8 (K >= 1, H * 3 / 2, W), got {tuple(chunk_u8.shape)} "
                             f"{chunk_u8.dtype}")
        K, (H, W, surf) = chunk_u8.shape[0], _yuv_geom(chunk_u8.shape, pixel_format, window, "chunk")
    else:
        check_window(chunk_u8.shape, pixel_format, window)
        if chunk_u8.dtype != torch.uint8 or chunk_u8.dim() != 4 or chunk_u8.shape[-1] != 3 or chunk_u8.shape[0] < 1:
            raise ValueError(f"chunk must be uint8 (K >= 1, H, W, 3), got {tuple(chunk_u8.shape)} {chunk_u8.dtype}")
        K, H, W, _ = chunk_u8.shape
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] > 65535:
        raise ValueError(f"pairs must be int32 (P <= 65535, 2) = frame in chunk, slot, got {tuple(pairs.shape)} {pairs.dtype}")
    if params_row.dtype != torch.int32 or tuple(params_row.shape) != (5,):
        raise ValueError(f"params_row must be int32 (5,), got {tuple(params_row.shape)} {params_row.dtype}")
    if ring.dtype != torch.float32 or ring.dim() != 4 or ring.shape[1] != 3 or ring.shape[2] != ring.shape[3] or \
            not ring.is_contiguous() or ring.data_ptr() % 16:
        raise ValueError(f"the ring must be contiguous, 16-byte aligned fp32 (R, 3, S, S), got {tuple(ring.shape)} {ring.dtype}")
    if W > 6000:
        raise ValueError(f"frames wider than 6000 pixels are not supported, got W {W}")
    _gpu(chunk_u8, pairs, params_row, ring)
    P, R, S = pairs.shape[0], ring.shape[0], ring.shape[2]
    if P == 0:
        return ring
    x = chunk_u8.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    f3 = C.c_float * 3
    tab, par = pairs.contiguous(), params_row.contiguous()
    with torch.cuda.device(ring.device):
        if surf:
            L.check(L.load().csts_stream_ingest_yuv_win(x.data_ptr(), K, H, W, *surf, tab.data_ptr(), P, par.data_ptr(),
                                                        ring.data_ptr(), R, S, f3(*mean), f3(*std), layout, mat, fr, _s()),
                    "csts_stream_ingest_yuv_win")
        elif layout:
            L.check(L.load().csts_stream_ingest_yuv(x.data_ptr(), K, H, W, tab.data_ptr(), P, par.data_ptr(), ring.data_ptr(), R, S,
                                                    f3(*mean), f3(*std), layout, mat, fr, _s()), "csts_stream_ingest_yuv")
        else:
            L.check(L.load().csts_stream_ingest(x.data_ptr(), K, H, W, tab.data_ptr(), P, par.data_ptr(), ring.data_ptr(), R, S,
                                                f3(*mean), f3(*std), _s()), "csts_stream_ingest")
    return ring


def stream_gather(ring: torch.Tensor, slots: torch.Tensor) -> torch.Tensor:
    """Clips out of the crop ring (csts_stream_gather): ring fp32 (R, 3, S, S), slots int32 (B, T) on the device -> fp32
    (B, 3, T, S, S), out[b, :, t] = ring[slots[b, t]].  The table is read by the kernel when it runs; a slot outside [0, R) gives
    a NaN frame."""
    _gpu(ring, slots)
    if ring.dtype != torch.float32 or ring.dim() != 4 or ring.shape[1] != 3 or ring.shape[2] != ring.shape[3] or \
            not ring.is_contiguous():
        raise ValueError(f"the ring must be contiguous fp32 (R, 3, S, S), got {tuple(ring.shape)} {ring.dtype}")
    if slots.dtype != torch.int32 or slots.dim() != 2:
        raise ValueError(f"slots must be int32 (B, T), got {tuple(slots.shape)} {slots.dtype}")
    B, T = slots.shape
    if not 1 <= T <= 64 or not 1 <= B <= 65535:
        raise ValueError(f"the gather takes 1 <= B <= 65535 clips of 1 <= T <= 64 frames, got B {B}, T {T}")
    R, S = ring.shape[0], ring.shape[2]
    out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=ring.device)
    with torch.cuda.device(ring.device):
        L.check(L.load().csts_stream_gather(ring.data_ptr(), R, slots.contiguous().data_ptr(), out.data_ptr(), B, T, S, _s()),
                "csts_stream_gather")
    return out


def _upload(device, *tables):
    """Host tables (numpy, any integer types) -> their device copies, by ONE host-to-device copy: the tables are laid out one
    after the other at 16-byte boundaries of one byte buffer and handed back as views of its device copy."""
    import numpy as np
    tables = [np.ascontiguousarray(t) for t in tables]
    offs, total = [], 0
    for t in tables:
        offs.append(total)
        total += (t.nbytes + 15) // 16 * 16
    host = np.zeros(max(total, 16), dtype=np.uint8)
    for t, o in zip(tables, offs):
        host[o:o + t.nbytes] = t.reshape(-1).view(np.uint8)
    dev = torch.from_numpy(host).to(device)
    return [dev[o:o + t.nbytes].view(getattr(torch, t.dtype.name)).reshape(t.shape) for t, o in zip(tables, offs)]


def _group_rings(rings, nbins=None):
    if rings.dtype != torch.float32 or rings.dim() != 3 or not rings.is_contiguous() or (nbins and rings.shape[1] != nbins):
        raise ValueError(f"the rings must be contiguous fp32 (streams, {nbins or 'nbins'}, ring_cols), got {tuple(rings.shape)} "
                         f"{rings.dtype}")
    return rings.shape


def group_stft(jobs, rings: torch.Tensor, n_fft: int = STFT_N_FFT, hop: int = STFT_HOP, win: int = STFT_WIN,
               eps: float = STFT_EPS) -> torch.Tensor:
    """stream_stft for several streams in ONE launch (csts_group_stft): jobs is a list of (buf, s_base, f0, f1, stream, n_total),
    each as stream_stft takes them -- buf fp32 (m,) on the device holds the samples [s_base, s_base + m) of that stream's signal,
    n_total -1 while it goes on -- and rings fp32 (streams, n_fft // 2 + 1, ring_cols) receives column f of stream i at
    rings[i, :, f % ring_cols], with stream_stft's bits.  A job may have f1 == f0 (it writes nothing); two jobs naming one
    stream, a stream outside the arena, a column that needs a sample its buffer does not hold or more than ring_cols columns
    in one job are a ValueError before anything is launched.  The job table goes up in one copy.  Returns the rings."""
    import numpy as np
    _gpu(rings)
    streams, _, ring_cols = _group_rings(rings, n_fft // 2 + 1)
    jobs = list(jobs)
    if not jobs:
        return rings
    table = np.zeros((len(jobs), 8), dtype=np.int64)
    keep, seen, total = [], set(), 0
    for j, (buf, s_base, f0, f1, slot, n_total) in enumerate(jobs):
        _gpu(buf)
        if buf.dtype != torch.float32 or buf.dim() != 1:
            raise ValueError(f"job {j}: buf must be an fp32 (m,) waveform, got {tuple(buf.shape)} {buf.dtype}")
        buf = buf.contiguous()
        keep.append(buf)
        s_base, f0, f1, slot, n_total, m = int(s_base), int(f0), int(f1), int(slot), int(n_total), buf.numel()
        if not 0 <= slot < streams or slot in seen:
            raise ValueError(f"job {j}: stream {slot} lies outside [0, {streams}) or is named by two jobs")
        seen.add(slot)
        if s_base < 0 or f0 < 0 or f1 < f0 or f1 - f0 > ring_cols:
            raise ValueError(f"job {j}: columns [{f0}, {f1}) must be at most one turn of the ring ({ring_cols} columns); s_base "
                             f"{s_base} >= 0")
        if n_total >= 0 and n_total > s_base + m:
            raise ValueError(f"job {j}: n_total {n_total} lies past the {s_base + m} samples pushed")
        first = max(f0 * hop + (n_fft - win) // 2 - n_fft // 2, 0)
        last = (f1 - 1) * hop + (n_fft - win) // 2 - n_fft // 2 + win
        if n_total >= 0:
            last = min(last, n_total)
        if f1 > f0 and last > first and (first < s_base or last > s_base + m):
            raise ValueError(f"job {j}: columns [{f0}, {f1}) read the samples [{first}, {last}), the buffer holds "
                             f"[{s_base}, {s_base + m})")
        table[j] = (buf.data_ptr() if m else 0, s_base, m, n_total, f0, f1, slot, total)
        total += f1 - f0
    if total == 0:
        return rings
    (dev,) = _upload(rings.device, table)
    with torch.cuda.device(rings.device):
        L.check(L.load().csts_group_stft(dev.data_ptr(), table.ctypes.data, len(jobs), rings.data_ptr(), streams, ring_cols, n_fft,
                                         hop, win, eps, _s()), "csts_group_stft")
    return rings


def group_audio_windows(rings: torch.Tensor, stream_of, newest, centers, width: int = 256, check: bool = True) -> torch.Tensor:
    """stream_audio_windows over the spectrum rings of a stream group (csts_group_audio_windows): rings fp32 (streams, nbins,
    ring_cols); stream_of (B,), newest (streams,) = the last column written of every stream (-1: none) and centers (B, T), GLOBAL
    centre columns, are HOST tables (anything numpy.asarray takes), which go up in one copy -> (B, 1, T, nbins, width): row b
    holds the windows of stream stream_of[b], read across that ring's wrap.  check: a row whose stream lies outside the arena, or
    a window not wholly inside its stream's live span [max(newest - ring_cols + 1, 0), newest], is a ValueError; with check=False
    it is left to the device, which applies the same test when the kernel runs and gives such a window NaN."""
    import numpy as np
    _gpu(rings)
    streams, nbins, ring_cols = _group_rings(rings)
    stream_of = np.asarray(stream_of, dtype=np.int32)
    newest = np.asarray(newest, dtype=np.int64)
    centers = np.asarray(centers, dtype=np.int64)
    width = int(width)
    if centers.ndim != 2 or stream_of.shape != centers.shape[:1] or newest.shape != (streams,):
        raise ValueError(f"stream_of must be (B,), newest ({streams},) and centers (B, T), got {stream_of.shape}, {newest.shape} and "
                         f"{centers.shape}")
    B, T = centers.shape
    if width < 2 or width % 2 or width > ring_cols or B < 1 or T < 1 or B * T > 65535:
        raise ValueError(f"bad sizes: width {width} (even, <= ring_cols {ring_cols}), B {B}, T {T} (B * T <= 65535)")
    if check:
        if int(stream_of.min()) < 0 or int(stream_of.max()) >= streams:
            raise ValueError(f"stream_of names a stream outside [0, {streams}): {stream_of.tolist()}")
        new = newest[stream_of][:, None]
        bad = (centers - width // 2 < np.maximum(new - ring_cols + 1, 0)) | (centers + width // 2 - 1 > new)
        if bad.any():
            b = int(np.argwhere(bad)[0][0])
            raise ValueError(f"an audio window of row {b} (stream {int(stream_of[b])}) reaches outside the ring's live columns "
                             f"[{max(int(new[b, 0]) - ring_cols + 1, 0)}, {int(new[b, 0])}] ({ring_cols} columns): centres "
                             f"{int(centers[b].min())} .. {int(centers[b].max())}, width {width}")
    d_new, d_cen, d_of = _upload(rings.device, newest, centers, stream_of)
    out = torch.empty(B, 1, T, nbins, width, dtype=torch.float32, device=rings.device)
    with torch.cuda.device(rings.device):
        L.check(L.load().csts_group_audio_windows(rings.data_ptr(), streams, ring_cols, d_of.data_ptr(), d_new.data_ptr(),
                                                  d_cen.data_ptr(), out.data_ptr(), B, T, nbins, width, _s()),
                "csts_group_audio_windows")
    return out


def group_ingest(jobs, pairs, arena: torch.Tensor, mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225), *,
                 pixel_format: str = "rgb24", matrix: str = "bt601", full_range: bool = False, window=None) -> torch.Tensor:
    """stream_ingest for several streams in ONE launch (csts_group_ingest / _yuv): jobs is a list of (chunk, params_row) -- chunk
    uint8 (K, H, W, 3) on the device, or (K, H * 3 / 2, W) in the one pixel_format of the call, each job of its own size;
    params_row the five test-mode integers new h, new w, y0, x0, flip of that job, on the HOST -- and pairs a HOST table (P, 3) =
    (job, frame in chunk, arena slot): arena fp32 (slots, 3, S, S) receives arena[slot] = clip_sample(chunk of the job,
    [[frame]], params_row[None], S)[0, :, 0], bit for bit.  A chunk frame no pair names is not read and no other slot is
    written; a pair whose job, frame or slot is out of range writes nothing; the tables go up in one copy and are read by the
    kernel when it runs.  A chunk that does not start at a 16-byte boundary is copied first, as stream_ingest does.  P == 0
    launches nothing.  The chunks are tight pictures: a window is refused.  Returns the arena."""
    import numpy as np
    no_window(window, "group_ingest")
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    if arena.dtype != torch.float32 or arena.dim() != 4 or arena.shape[1] != 3 or arena.shape[2] != arena.shape[3] or \
            not arena.is_contiguous() or arena.data_ptr() % 16:
        raise ValueError(f"the arena must be contiguous, 16-byte aligned fp32 (slots, 3, S, S), got {tuple(arena.shape)} {arena.dtype}")
    _gpu(arena)
    jobs = list(jobs)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 3)
    if pairs.shape[0] > 65535 or len(jobs) > 65535:
        raise ValueError(f"a launch takes at most 65535 jobs and pairs, got {len(jobs)} and {pairs.shape[0]}")
    if pairs.shape[0] == 0 or not jobs:
        return arena
    table = np.zeros((len(jobs), 6), dtype=np.int64)
    params = np.zeros((len(jobs), 5), dtype=np.int32)
    keep = []
    for j, (chunk, row) in enumerate(jobs):
        _gpu(chunk)
        if layout:
            if chunk.dtype != torch.uint8 or chunk.dim() != 3 or chunk.shape[0] < 1:
                raise ValueError(f"job {j}: {pixel_format} chunk must be uint8 (K >= 1, H * 3 / 2, W), got {tuple(chunk.shape)} "
                                 f"{chunk.dtype}")
            K, (H, W) = chunk.shape[0], _yuv_hw(chunk.shape, pixel_format, "chunk")
            cap = (W + 30 + 15) // 16 * 16
        else:
            if chunk.dtype != torch.uint8 or chunk.dim() != 4 or chunk.shape[-1] != 3 or chunk.shape[0] < 1:
                raise ValueError(f"job {j}: chunk must be uint8 (K >= 1, H, W, 3), got {tuple(chunk.shape)} {chunk.dtype}")
            K, H, W, _ = chunk.shape
            cap = (3 * W + 30 + 15) // 16 * 16
        if W > 6000:
            raise ValueError(f"job {j}: frames wider than 6000 pixels are not supported, got W {W}")
        x = chunk.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        keep.append(x)
        table[j] = (x.data_ptr(), x.numel(), K, H, W, cap)
        params[j] = np.asarray(row, dtype=np.int32).reshape(5)
    d_jobs, d_params, d_pairs = _upload(arena.device, table, params, pairs)
    f3 = C.c_float * 3
    args = (d_jobs.data_ptr(), table.ctypes.data, len(jobs), d_params.data_ptr(), d_pairs.data_ptr(), pairs.shape[0], arena.data_ptr(),
            arena.shape[0], arena.shape[2], f3(*mean), f3(*std))
    with torch.cuda.device(arena.device):
        if layout:
            L.check(L.load().csts_group_ingest_yuv(*args, layout, mat, fr, _s()), "csts_group_ingest_yuv")
        else:
            L.check(L.load().csts_group_ingest(*args, _s()), "csts_group_ingest")
    return arena


def _clip_table(clips, B=None):
    """The clip table {byte offset, N, H, W} as a contiguous int64 (B, 4) tensor; the caller validates its rows."""
    if clips.dtype != torch.int64 or clips.dim() != 2 or clips.shape[1] != 4 or clips.shape[0] < 1 or \
            (B is not None and clips.shape[0] != B):
        raise ValueError(f"clips must be int64 ({'B' if B is None else B}, 4) = byte offset, N, H, W, got {tuple(clips.shape)} "
                         f"{clips.dtype}")
    return clips.contiguous()


def batch_params(labels: torch.Tensor, clips: torch.Tensor, crop_size: int, *, train: bool, min_scale: int = 0, max_scale: int = 0,
                 spatial_idx: int = 1, random_flip: bool = True, inverse_uniform: bool = False, generator=None,
                 key: torch.Tensor = None, clips_host=None):
    """The rule pass of spatial_sampling for clips of B recordings of B frame sizes (csts_batch_params): labels floating
    (B, T, L >= 2), clips int64 (B, 4) = {byte offset, N, H, W} on the device (H, W are read there) -> (params int32 (B, 5),
    labels fp64 (B, T, L)).  Clip b draws the variates u[b] under the key (drawn from `generator` as spatial_sampling draws it,
    or given), so with equal sizes the result is spatial_sampling's.  clips_host: the same table on the host (anything
    numpy.asarray takes); given, its H, W are validated without a device read (ValueError)."""
    if labels.dim() != 3 or labels.shape[2] < 2 or not labels.is_floating_point():
        raise ValueError(f"labels must be floating (B, T, L >= 2), got {tuple(labels.shape)} {labels.dtype}")
    B, T, ncol = labels.shape
    tab = _clip_table(clips, B)
    S = int(crop_size)
    if not 1 <= T <= 64:
        raise ValueError(f"spatial sampling takes 1 <= T <= 64 frames per clip, got {T}")
    if S < 1:
        raise ValueError(f"crop_size must be positive, got {S}")
    if train:
        min_scale, max_scale = int(min_scale), int(max_scale)
        if min_scale < S:
            raise ValueError(f"the short side would end up below the crop: min_scale {min_scale} < crop_size {S}")
        if max_scale < min_scale:
            raise ValueError(f"max_scale {max_scale} < min_scale {min_scale}")
        idx = -1
    else:
        idx = int(spatial_idx)
        if idx not in (0, 1, 2):
            raise ValueError(f"spatial_idx must be 0, 1 or 2 in test mode, got {spatial_idx}")
    if clips_host is not None:
        import numpy as np
        hw = np.asarray(clips_host).reshape(-1, 4)[:, 2:]
        if hw.shape[0] != B or int(hw.min()) < 1:
            raise ValueError(f"the clip table must hold {B} rows with H, W >= 1, got {hw.tolist()}")
    _gpu(labels, tab)
    lab = labels.to(torch.float64).contiguous()
    dev = lab.device
    if not train:
        key = None
    elif key is None:
        key = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=dev, generator=generator)
    elif key.dtype != torch.int64 or key.numel() != 1 or key.device != dev:
        raise ValueError("key must be an int64 tensor of one element on the labels' device")
    params = torch.empty(B, 5, dtype=torch.int32, device=dev)
    new_labels = torch.empty_like(lab)
    L.check(L.load().csts_batch_params(key.data_ptr() if key is not None else None, lab.data_ptr(), tab.data_ptr(), B, T, ncol, S,
                                       min_scale, max_scale, idx, int(bool(random_flip)), int(bool(inverse_uniform)),
                                       params.data_ptr(), new_labels.data_ptr(), _s()), "csts_batch_params")
    return params, new_labels


def batch_sample(arena_u8: torch.Tensor, clips: torch.Tensor, frames_idx: torch.Tensor, params: torch.Tensor, crop_size: int,
                 clips_host, mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225), out: torch.Tensor = None, *,
                 pixel_format: str = "rgb24", matrix: str = "bt601", full_range: bool = False, window=None) -> torch.Tensor:
    """clip_sample for clips of B different recordings in ONE launch (csts_batch_sample): arena_u8 uint8 (bytes,) holds the
    recordings back to back at any byte, clips int64 (B, 4) = {byte offset, N, H, W} on the device, frames_idx int32 (B, T)
    (clamped to [0, N_b - 1] on the device), params int32 (B, 5) -> fp32 (B, 3, T, S, S); clip b is, bit for bit,
    clip_sample(recording_b, frames_idx[b:b+1], params[b:b+1], S).  clips_host: the table on the host; every row must lie inside
    the arena with N, H, W >= 1 (ValueError) -- the device reads the tables when the kernel runs and gives a NaN clip for a row
    that does not, so a captured launch stays safe when the tables are rewritten.  pixel_format "nv12" | "i420": the recordings
    are 4:2:0 pictures (csts_batch_sample_yuv); the table keeps its columns with H the luma height (H, W even), a recording
    occupies N H W 3 / 2 bytes and clip b is clip_sample of it in that format.  The recordings are tight: a window is refused."""
    import numpy as np
    no_window(window, "batch_sample")
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    if arena_u8.dtype != torch.uint8 or arena_u8.dim() != 1 or arena_u8.numel() < 3:
        raise ValueError(f"the arena must be uint8 (bytes,), got {tuple(arena_u8.shape)} {arena_u8.dtype}")
    if frames_idx.dtype != torch.int32 or frames_idx.dim() != 2:
        raise ValueError(f"frames_idx must be int32 (B, T), got {tuple(frames_idx.shape)} {frames_idx.dtype}")
    B, T = frames_idx.shape
    if not 1 <= T <= 64 or B < 1:
        raise ValueError(f"clip sampling takes B >= 1 clips of 1 <= T <= 64 frames, got B {B}, T {T}")
    tab = _clip_table(clips, B)
    if params.dtype != torch.int32 or tuple(params.shape) != (B, 5):
        raise ValueError(f"params must be int32 ({B}, 5), got {tuple(params.shape)} {params.dtype}")
    S = int(crop_size)
    if S < 1:
        raise ValueError(f"crop_size must be positive, got {S}")
    host = np.asarray(clips_host, dtype=np.int64).reshape(-1, 4)
    if host.shape[0] != B:
        raise ValueError(f"the host clip table has {host.shape[0]} rows, the batch {B}")
    nbytes = arena_u8.numel()
    for b, (off, n, h, w) in enumerate(host.tolist()):
        if layout and (h % 2 or w % 2):
            raise ValueError(f"clip {b}: {pixel_format} recordings need even H and W, got H {h}, W {w}")
        if n < 1 or h < 1 or w < 1 or w > 6000 or off < 0 or off + (n * h * w * 3 // 2 if layout else n * h * w * 3) > nbytes:
            raise ValueError(f"clip {b}: recording (offset {off}, N {n}, H {h}, W {w}) does not lie inside the arena of {nbytes} "
                             "bytes (or W > 6000)")
    _gpu(arena_u8, tab, frames_idx, params)
    if not arena_u8.is_contiguous() or arena_u8.data_ptr() % 16:
        raise ValueError("the arena must be contiguous and 16-byte aligned")
    if out is None:
        out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=arena_u8.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, T, S, S) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"out must be a contiguous fp32 ({B}, 3, {T}, {S}, {S}) GPU tensor")
    f3 = C.c_float * 3
    idx, par = frames_idx.contiguous(), params.contiguous()
    if layout:
        L.check(L.load().csts_batch_sample_yuv(arena_u8.data_ptr(), nbytes, tab.data_ptr(), idx.data_ptr(), par.data_ptr(),
                                               out.data_ptr(), B, T, S, int(host[:, 3].max()), f3(*mean), f3(*std), layout, mat, fr,
                                               _s()), "csts_batch_sample_yuv")
        return out
    L.check(L.load().csts_batch_sample(arena_u8.data_ptr(), nbytes, tab.data_ptr(), idx.data_ptr(), par.data_ptr(), out.data_ptr(),
                                       B, T, S, int(host[:, 3].max()), f3(*mean), f3(*std), _s()), "csts_batch_sample")
    return out


def audio_gather(spec_arena: torch.Tensor, specs: torch.Tensor, centers: torch.Tensor, nbins: int, specs_host, width: int = 256,
                 out: torch.Tensor = None) -> torch.Tensor:
    """audio_windows_at for clips of B different recordings in ONE launch (csts_audio_gather): spec_arena fp32 (floats,) holds
    one (nbins, stride_b) spectrogram per clip, specs int64 (B, 3) = {float offset, row stride, usable columns} on the device,
    centers int32 (B, T) -> (B, 1, T, nbins, width); window (b, t) = spec_b[:, c - width/2 : c + width/2], c clamped to
    [width/2, usable_b - 1 - width/2] on the device: audio_windows_at(spec_b[:, :usable_b], centers[b:b+1]).  specs_host: the
    table on the host, validated against the arena (ValueError)."""
    import numpy as np
    if spec_arena.dtype != torch.float32 or spec_arena.dim() != 1:
        raise ValueError(f"the spectrogram arena must be fp32 (floats,), got {tuple(spec_arena.shape)} {spec_arena.dtype}")
    if centers.dtype != torch.int32 or centers.dim() != 2:
        raise ValueError(f"centers must be int32 (B, T), got {tuple(centers.shape)} {centers.dtype}")
    B, T = centers.shape
    if specs.dtype != torch.int64 or tuple(specs.shape) != (B, 3):
        raise ValueError(f"specs must be int64 ({B}, 3) = float offset, row stride, usable columns, got {tuple(specs.shape)} "
                         f"{specs.dtype}")
    nbins, width = int(nbins), int(width)
    if nbins < 1 or width < 2 or width % 2 or B < 1 or T < 1 or B * T > 65535:
        raise ValueError(f"bad sizes: nbins {nbins}, width {width} (even), B {B}, T {T} (B * T <= 65535)")
    host = np.asarray(specs_host, dtype=np.int64).reshape(-1, 3)
    if host.shape[0] != B:
        raise ValueError(f"the host spectrogram table has {host.shape[0]} rows, the batch {B}")
    nfl = spec_arena.numel()
    for b, (off, stride, usable) in enumerate(host.tolist()):
        if off < 0 or usable > stride or off + nbins * stride > nfl:
            raise ValueError(f"clip {b}: spectrogram (offset {off}, stride {stride}, usable {usable}) does not lie inside the arena "
                             f"of {nfl} floats")
        if usable < width + 1:
            raise ValueError(f"clip {b}: the spectrogram has {usable} usable columns, a window needs {width + 1}")
    _gpu(spec_arena, specs, centers)
    if not spec_arena.is_contiguous():
        raise ValueError("the spectrogram arena must be contiguous")
    if out is None:
        out = torch.empty(B, 1, T, nbins, width, dtype=torch.float32, device=spec_arena.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 1, T, nbins, width) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"out must be a contiguous fp32 ({B}, 1, {T}, {nbins}, {width}) GPU tensor")
    L.check(L.load().csts_audio_gather(spec_arena.data_ptr(), specs.contiguous().data_ptr(), centers.contiguous().data_ptr(),
                                       out.data_ptr(), B, T, nbins, width, _s()), "csts_audio_gather")
    return out


def spatial_rule_host(labels, H: int, W: int, crop_size: int, *, train: bool, uniforms=None, min_scale: int = 0,
                      max_scale: int = 0, spatial_idx: int = 1, random_flip: bool = True, inverse_uniform: bool = False):
    """The rule of spatial_sampling on the CPU (csts_spatial_rule_host) from explicit variates: labels float64 (B, T, L),
    uniforms float64 (B, 4) (train) -> (params int32 (B, 5) = new h, new w, y0, x0, flip, labels float64 (B, T, L))."""
    import numpy as np
    lab = np.ascontiguousarray(labels, dtype=np.float64)
    if lab.ndim != 3:
        raise ValueError(f"labels must be (B, T, L), got shape {lab.shape}")
    B, T, ncol = lab.shape
    u = None
    if train:
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        if u.shape != (B, 4):
            raise ValueError(f"uniforms must be ({B}, 4), got {u.shape}")
    params = np.zeros((B, 5), dtype=np.int32)
    out = np.zeros_like(lab)
    L.check(L.load().csts_spatial_rule_host(lab.ctypes.data, B, T, ncol, H, W, int(crop_size), int(min_scale), int(max_scale),
                                            -1 if train else int(spatial_idx), int(bool(random_flip)), int(bool(inverse_uniform)),
                                            u.ctypes.data if u is not None else None, params.ctypes.data, out.ctypes.data),
            "csts_spatial_rule_host")
    return params, out


def spatial_uniforms_host(key: int, first: int, count: int):
    """The variates u0..u3 (float64 (count, 4)) spatial_sampling draws for clips first .. first + count - 1 under a 64-bit key
    (csts_spatial_uniforms_host)."""
    import numpy as np
    key &= (1 << 64) - 1
    out = np.zeros((count, 4), dtype=np.float64)
    L.check(L.load().csts_spatial_uniforms_host(key & 0xFFFFFFFF, key >> 32, first, count, out.ctypes.data),
            "csts_spatial_uniforms_host")
    return out


def assemble_batch(frames_u8, wav, frames_idx, frame_length, labels, spatial=None, *, pixel_format: str = "rgb24",
                   matrix: str = "bt601", full_range: bool = False, window=None):
    """uint8 frames (B, T, H, W, 3), waveform (B, n), sampled frame indices (B, T), gaze labels (B, T, 3) -> the batch
    dict the training step takes (video, audio, labels_hm, labels).  spatial: None (frames normalised at the size they
    come in), or the keyword arguments of spatial_sampling (crop_size, train, ...): the video is spatially sampled, and
    the heat maps ((S/4)^2) and the returned labels are the transformed ones (ego4d_avgaze_forecast.py:302-326).
    pixel_format "nv12" | "i420": the frames are 4:2:0 pictures uint8 (B, T, H * 3 / 2, W); with spatial they are sampled in
    place, without it they are converted (yuv_to_rgb) and normalised; window (top, left, H, W): they are surfaces (B, T,
    Hs * 3 / 2, Ws) and the pictures their windows, read in place either way."""
    yuv = check_pixel_format(pixel_format, matrix, full_range)[0] != 0
    fmt = dict(pixel_format=pixel_format, matrix=matrix, full_range=full_range, window=window) if yuv else {}
    if yuv:
        if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
            raise ValueError(f"{pixel_format} frames must be uint8 (B, T, H * 3 / 2, W), got {tuple(frames_u8.shape)}")
        _yuv_hw(frames_u8.shape, pixel_format)
        check_window(frames_u8.shape, pixel_format, window)
    else:
        check_window(getattr(frames_u8, "shape", ()), pixel_format, window)
    if spatial is None:
        return {"video": normalize_frames(yuv_to_rgb(frames_u8, **fmt) if yuv else frames_u8),
                "audio": audio_windows(stft_logpower(wav), frames_idx, frame_length),
                "labels_hm": gaze_heatmaps(labels), "labels": labels}
    kw = dict(spatial)
    S = int(kw.pop("crop_size"))
    video, new_labels = spatial_sampling(frames_u8, labels, S, **kw, **fmt)
    return {"video": video,
            "audio": audio_windows(stft_logpower(wav), frames_idx, frame_length),
            "labels_hm": gaze_heatmaps(new_labels, H=S // 4, W=S // 4), "labels": new_labels}
