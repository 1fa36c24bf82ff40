"""The four stream kernels alone (no model), every comparison torch.equal against an existing op: stream_stft against
stft_logpower of the whole waveform, stream_audio_windows against audio_windows_at on the offline spectrogram, stream_ingest +
stream_gather against clip_sample of the concatenated video."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import inputs  # noqa: E402

DEV = torch.device("cuda:0")
N_WAV, RING_COLS = 90000, 512


@pytest.fixture(scope="module")
def audio():
    """The waveform, its offline spectrogram (750 columns), and the ring after the whole waveform went through it in ragged pieces;
    `seen` holds every column as it was read back right after the push that wrote it."""
    g = torch.Generator().manual_seed(3)
    wav = (0.1 * torch.randn(N_WAV, generator=g)).to(DEV)
    spec = inputs.stft_logpower(wav[None])[0]
    assert spec.shape == (256, 750)
    ring = torch.full((256, RING_COLS), float("nan"), dtype=torch.float32, device=DEV)
    seen = torch.full_like(spec, float("nan"))
    sizes = [1, 119, 1, 120, 239, 241, 7, 5000, 119, 1, 30000, 1, 1, 12345]
    pos = cols = base = 0
    tail = wav[:0]
    mid = None
    pieces = 0
    while pos < N_WAV:
        m = min(sizes[pieces % len(sizes)], N_WAV - pos)
        pieces += 1
        buf = torch.cat([tail, wav[pos:pos + m]])
        pos += m
        new = pos // 120
        if new > cols:
            assert new - cols <= RING_COLS
            inputs.stream_stft(buf, base, cols, new, ring)
            seen[:, cols:new] = ring[:, torch.arange(cols, new, device=DEV) % RING_COLS]
            cols = new
            if mid is None and cols > RING_COLS + 100:
                mid = (cols, ring.clone())                       # a state in which the ring has wrapped
        keep = max(0, 120 * cols - 120, base)
        assert pos - keep < 240                                   # the tail the unfinished columns need
        tail, base = buf[keep - base:].clone(), keep
    assert cols == 750 > RING_COLS and mid is not None
    return {"wav": wav, "spec": spec, "ring": ring, "seen": seen, "mid": mid, "tail": (tail, base)}


def test_every_column_equals_the_offline_column(audio):
    # 90 000 samples are 750 hops: the running stream has every offline column and close() has nothing to add
    assert not bool(torch.isnan(audio["seen"]).any())
    assert torch.equal(audio["seen"], audio["spec"])
    live = torch.arange(750 - RING_COLS, 750, device=DEV)
    assert torch.equal(audio["ring"][:, live % RING_COLS], audio["spec"][:, live])


def test_close_adds_the_offline_tail_and_touches_no_other_column(audio):
    n = N_WAV - 50                                                # no multiple of the hop: the offline STFT has one more column
    wav = audio["wav"][:n]
    spec = inputs.stft_logpower(wav[None])[0]
    assert spec.shape == (256, 750) and n // 120 == 749
    ring = torch.full((256, RING_COLS), float("nan"), dtype=torch.float32, device=DEV)
    inputs.stream_stft(wav[:60000], 0, 0, 500, ring)
    inputs.stream_stft(wav[60000 - 120:], 60000 - 120, 500, 749, ring)
    before = ring.clone()
    tail = wav[120 * 749 - 120:].clone()
    assert tail.numel() == 190
    inputs.stream_stft(tail, 120 * 749 - 120, 749, 750, ring, n_total=n)      # what close() adds: zeros past the last sample
    assert torch.equal(ring[:, 749 % RING_COLS], spec[:, 749])
    others = torch.arange(RING_COLS, device=DEV) != 749 % RING_COLS
    assert torch.equal(ring[:, others], before[:, others])
    live = torch.arange(750 - RING_COLS, 750, device=DEV)
    assert torch.equal(ring[:, live % RING_COLS], spec[:, live])
    assert not torch.equal(spec[:, 749], audio["spec"][:, 749])  # the padded column is not the running one


def test_stft_refuses_columns_the_buffer_does_not_cover(audio):
    tail, base = audio["tail"]
    ring = torch.zeros(256, RING_COLS, device=DEV)
    with pytest.raises(ValueError, match="the buffer holds"):
        inputs.stream_stft(tail, base, 750, 751, ring)            # the column needs samples past the end
    with pytest.raises(ValueError, match="the buffer holds"):
        inputs.stream_stft(tail, base, 748, 750, ring)            # samples already dropped
    with pytest.raises(ValueError, match="one turn"):
        inputs.stream_stft(audio["wav"], 0, 0, RING_COLS + 1, ring)


def test_windows_across_the_wrap_equal_audio_windows_at(audio):
    spec = audio["spec"]
    newest, ring = audio["mid"][0] - 1, audio["mid"][1]
    wrap = (newest // RING_COLS) * RING_COLS                      # global column that sits at ring column 0
    oldest = newest - RING_COLS + 1
    assert oldest + 129 < wrap - 127 and wrap + 1 <= newest - 127
    cen = np.array([[oldest + 128, wrap - 127, wrap - 1, wrap], [wrap + 1, newest - 127, wrap - 64, oldest + 129]], dtype=np.int64)
    assert int((cen - 128 < wrap).sum()) == 8 and int((cen + 127 >= wrap).sum()) == 6      # six windows cross the wrap position
    got = inputs.stream_audio_windows(ring, newest, torch.from_numpy(cen).to(DEV), cen)
    want = inputs.audio_windows_at(spec, torch.from_numpy(cen).to(DEV).to(torch.int32))    # none of these centres is clamped
    assert 128 <= int(cen.min()) and int(cen.max()) <= spec.shape[1] - 1 - 128
    assert got.shape == (2, 1, 4, 256, 256) and torch.equal(got, want)
    # the final ring, read at its oldest and newest live columns (audio_windows_at would clamp the newest: slices instead)
    cen = np.array([[750 - 128, 750 - RING_COLS + 128]], dtype=np.int64)
    got = inputs.stream_audio_windows(audio["ring"], 749, torch.from_numpy(cen).to(DEV), cen)
    for t, c in enumerate(cen[0].tolist()):
        assert torch.equal(got[0, 0, t], spec[:, c - 128:c + 128])


def test_a_centre_outside_the_live_span_is_refused_and_nan_on_the_device(audio):
    newest, ring = audio["mid"][0] - 1, audio["mid"][1]
    oldest = newest - RING_COLS + 1
    for c in (oldest + 127, newest - 126, newest + 500, 0):
        cen = np.array([[c]], dtype=np.int64)
        with pytest.raises(ValueError, match="live columns"):
            inputs.stream_audio_windows(ring, newest, torch.from_numpy(cen).to(DEV), cen)
    # the device applies the same test to the table it reads: a stale host copy cannot make it read a dead column
    ok = np.array([[oldest + 128, newest - 127]], dtype=np.int64)
    dev = torch.tensor([[oldest + 127, newest - 127]], dtype=torch.int64, device=DEV)
    got = inputs.stream_audio_windows(ring, newest, dev, ok)
    assert bool(torch.isnan(got[0, 0, 0]).all()) and bool(torch.isfinite(got[0, 0, 1]).all())


# ---- ingest + gather ---------------------------------------------------------------------------------------------------------------
R, S = 12, 32
CHUNKS = [1, 5, 11, 1, 5, 11]                                     # 34 frames: the slot sequence f mod 12 wraps twice


def _video(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(DEV)


def _row(H, W):
    return inputs.spatial_rule_host(np.zeros((1, 8, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()


@pytest.mark.parametrize("fmt, shape, row", [
    ("rgb24", (34, 35, 51, 3), None),                            # 35 * 51 * 3 = 5355 bytes a frame: misaligned frame bases
    ("nv12", (34, 54, 52), None),                                # 36 x 52
    ("i420", (34, 54, 52), None),
    ("rgb24", (34, S, S, 3), [S, S, 0, 0, 0]),                   # the identity source
    ("rgb24", (34, 40, 64, 3), [48, 77, 9, 30, 1]),              # resize, crop and flip
])
def test_ingest_and_gather_equal_clip_sample_of_the_concatenated_video(fmt, shape, row):
    video = _video(shape, 7)
    kw = {} if fmt == "rgb24" else {"pixel_format": fmt, "matrix": "bt709", "full_range": True}
    H, W = (shape[1], shape[2]) if fmt == "rgb24" else (shape[1] * 2 // 3, shape[2])
    row = _row(H, W) if row is None else row
    assert row[0] >= S and row[1] >= S
    params = torch.tensor(row, dtype=torch.int32, device=DEV)
    N = shape[0]
    want = inputs.clip_sample(video, torch.arange(N, dtype=torch.int32, device=DEV)[None], params[None], S, **kw)[0]   # (3, N, S, S)
    ring = torch.full((R, 3, S, S), -7.0, dtype=torch.float32, device=DEV)
    used = [f for f in range(N) if f % 3 != 1]                   # every third frame is read by no window
    a = 0
    for k in CHUNKS:
        chunk = video[a:a + k]
        mine = [f for f in used if a <= f < a + k]
        before = ring.clone()
        pairs = torch.tensor([[f - a, f % R] for f in mine], dtype=torch.int32, device=DEV).reshape(-1, 2)
        inputs.stream_ingest(chunk, pairs, params, ring, **kw)
        touched = sorted({f % R for f in mine})
        rest = [r for r in range(R) if r not in touched]
        assert torch.equal(ring[rest], before[rest])              # a frame not in the table leaves the ring as it was
        for f in mine:
            assert torch.equal(ring[f % R], want[:, f]), (fmt, f)
        a += k
        # gather what is live: the last frames written to each slot, in a (B, T) table that repeats and reorders them
        live = {}
        for f in used:
            if f < a:
                live[f % R] = f
        frames = sorted(live.values())
        if len(frames) >= 4:
            tab = np.array([frames[:4], frames[-4:][::-1], [frames[0]] * 4], dtype=np.int64)
            got = inputs.stream_gather(ring, torch.from_numpy((tab % R).astype(np.int32)).to(DEV))
            ref = inputs.clip_sample(video, torch.from_numpy(tab.astype(np.int32)).to(DEV), params[None].repeat(3, 1), S, **kw)
            assert got.shape == (3, 3, 4, S, S) and torch.equal(got, ref), (fmt, a)
    assert a == N


def test_guards_write_nothing_and_a_bad_slot_gathers_nan():
    video = _video((4, 35, 51, 3), 9)
    params = torch.tensor(_row(35, 51), dtype=torch.int32, device=DEV)
    ring = torch.full((R, 3, S, S), 2.5, dtype=torch.float32, device=DEV)
    pairs = torch.tensor([[4, 0], [-1, 1], [0, R], [1, -1], [2, 5]], dtype=torch.int32, device=DEV)
    inputs.stream_ingest(video, pairs, params, ring)
    others = [r for r in range(R) if r != 5]
    assert bool((ring[others] == 2.5).all()) and not bool((ring[5] == 2.5).any())
    assert inputs.stream_ingest(video, pairs[:0], params, ring) is ring          # an empty table launches nothing
    got = inputs.stream_gather(ring, torch.tensor([[5, R, -1, 0]], dtype=torch.int32, device=DEV))
    assert torch.equal(got[0, :, 0], ring[5]) and torch.equal(got[0, :, 3], ring[0])
    assert bool(torch.isnan(got[0, :, 1]).all()) and bool(torch.isnan(got[0, :, 2]).all())
    bad = torch.tensor([S - 1, S, 0, 0, 0], dtype=torch.int32, device=DEV)       # parameters outside the rule's range: a NaN slot
    inputs.stream_ingest(video, torch.tensor([[0, 3]], dtype=torch.int32, device=DEV), bad, ring)
    assert bool(torch.isnan(ring[3]).all()) and bool((ring[2] == 2.5).all())
