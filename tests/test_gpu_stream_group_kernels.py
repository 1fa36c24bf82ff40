"""The group kernels alone (no model), every comparison torch.equal against the single-stream kernel on a ring of its own:
group_ingest against stream_ingest, group_stft against stream_stft (and stft_logpower), group_audio_windows against
stream_audio_windows.  The arenas are pre-filled with a sentinel, so equality with sentinel-filled single rings also shows that no
slot, column or byte outside what the tables name is written.  Crop slots and source sizes: 0: 64 x 80; 1: 48 x 62 (a width that is
no multiple of 4; 48 x 64 in the 4:2:0 cases); 2: 70 x 100 (another LDS row capacity in the same launch).  The STFT test uses four
spectrum rings: jobs of 0, 1, 7 and ring_cols columns in one launch name four streams."""
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
R, S, N = 12, 32, 17
SIZES = {"rgb24": [(64, 80), (48, 62), (70, 100)], "nv12": [(64, 80), (48, 64), (70, 100)], "i420": [(64, 80), (48, 64), (70, 100)]}
ROUNDS = [(1, 5, 11), (5, 11, 1), (11, 1, 5)]                    # chunk sizes of slots 0, 1, 2 in the three launches: 17 frames each
SENTINEL = -7.0


def _row(H, W):
    return inputs.spatial_rule_host(np.zeros((1, 8, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()


@pytest.mark.parametrize("fmt", ["rgb24", "nv12", "i420"])
def test_group_ingest_equals_stream_ingest_per_slot_and_writes_nothing_else(fmt):
    kw = {} if fmt == "rgb24" else {"pixel_format": fmt, "matrix": "bt709", "full_range": True}
    g = torch.Generator().manual_seed(11)
    videos, rows = [], []
    for H, W in SIZES[fmt]:
        shape = (N, H, W, 3) if fmt == "rgb24" else (N, H * 3 // 2, W)
        videos.append(torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(DEV))
        rows.append(_row(H, W))
    assert videos[2][1:].data_ptr() % 16 != 0 or fmt != "rgb24"  # 70 x 100 x 3 = 21 000 bytes a frame: a misaligned piece
    arena = torch.full((3 * R, 3, S, S), SENTINEL, dtype=torch.float32, device=DEV)
    rings = [torch.full((R, 3, S, S), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(3)]
    used = [f for f in range(N) if f % 3 != 1]                   # every third frame is read by no window, as with used_frames
    at = [0, 0, 0]
    for sizes in ROUNDS:
        jobs, pairs = [], []
        for i, k in enumerate(sizes):
            a = at[i]
            chunk = videos[i][a:a + k]
            mine = [f for f in used if a <= f < a + k]
            if mine:                                             # a chunk of one unused frame is no job (and no launch alone)
                ref = torch.tensor([[f - a, f % R] for f in mine], dtype=torch.int32, device=DEV)
                inputs.stream_ingest(chunk, ref, torch.tensor(rows[i], dtype=torch.int32, device=DEV), rings[i], **kw)
            pairs += [(len(jobs), f - a, i * R + f % R) for f in mine]
            jobs.append((chunk, rows[i]))
            at[i] += k
        # one pair each with a bad job, a bad frame and a bad arena slot: they write nothing
        pairs += [(3, 0, 0), (-1, 0, 1), (0, sizes[0], 2), (1, -1, 3), (2, 0, 3 * R), (2, 0, -1)]
        assert inputs.group_ingest(jobs, pairs, arena, **kw) is arena
        for i in range(3):
            assert torch.equal(arena[i * R:(i + 1) * R], rings[i]), (fmt, sizes, i)
    assert at == [N, N, N]
    assert int((arena == SENTINEL).all(dim=3).all(dim=2).all(dim=1).sum()) == 3 * sum(1 for r in range(R) if r not in {f % R for f in used})
    # the crops are clip_sample's: slot 1, frame 15 sits in arena slot R + 3
    want = inputs.clip_sample(videos[1], torch.tensor([[15]], dtype=torch.int32, device=DEV),
                              torch.tensor([rows[1]], dtype=torch.int32, device=DEV), S, **kw)[0, :, 0]
    assert torch.equal(arena[R + 15 % R], want)


def test_group_ingest_bad_params_give_a_nan_slot_and_an_empty_table_launches_nothing():
    g = torch.Generator().manual_seed(12)
    a = torch.randint(0, 256, (2, 64, 80, 3), generator=g, dtype=torch.uint8).to(DEV)
    b = torch.randint(0, 256, (3, 48, 62, 3), generator=g, dtype=torch.uint8).to(DEV)
    arena = torch.full((3 * R, 3, S, S), 2.5, dtype=torch.float32, device=DEV)
    assert inputs.group_ingest([(a, _row(64, 80))], [], arena) is arena and bool((arena == 2.5).all())
    inputs.group_ingest([(a, [S - 1, S, 0, 0, 0]), (b, _row(48, 62))], [(0, 1, 5), (1, 2, R + 7)], arena)
    assert bool(torch.isnan(arena[5]).all()) and bool(torch.isfinite(arena[R + 7]).all()) and not bool((arena[R + 7] == 2.5).any())
    others = [r for r in range(3 * R) if r not in (5, R + 7)]
    assert bool((arena[others] == 2.5).all())
    with pytest.raises(ValueError, match="6000"):
        inputs.group_ingest([(torch.zeros(1, 2, 6001, 3, dtype=torch.uint8, device=DEV), [S, S, 0, 0, 0])], [(0, 0, 0)], arena)


# ---- audio -------------------------------------------------------------------------------------------------------------------------
N_WAV, RING_COLS = 90000, 512


@pytest.fixture(scope="module")
def audio():
    g = torch.Generator().manual_seed(4)
    wavs = [(0.1 * torch.randn(N_WAV, generator=g)).to(DEV) for _ in range(4)]
    specs = [inputs.stft_logpower(w[None])[0] for w in wavs]
    assert specs[0].shape == (256, 750)
    return {"wavs": wavs, "specs": specs}


def test_group_stft_equals_stream_stft_per_ring(audio):
    wavs, specs = audio["wavs"], audio["specs"]
    arena = torch.full((4, 256, RING_COLS), SENTINEL, dtype=torch.float32, device=DEV)
    rings = [torch.full((256, RING_COLS), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(4)]
    n_end = 60050                                                # stream 1 ends here: no multiple of the hop, 501 offline columns
    offline = inputs.stft_logpower(wavs[1][None, :n_end])[0]
    assert offline.shape == (256, 501) and n_end // 120 == 500

    def both(jobs):
        """One group launch against one stream_stft call per job with columns, on that stream's own ring."""
        inputs.group_stft(jobs, arena)
        for buf, base, f0, f1, i, n_total in jobs:
            if f1 > f0:
                inputs.stream_stft(buf.contiguous(), base, f0, f1, rings[i], n_total=n_total)
        for i in range(4):
            assert torch.equal(arena[i], rings[i]), i

    def cut(i, f0, f1, end=None):
        """The samples columns [f0, f1) of stream i read, as a buffer that starts where column f0 starts."""
        base = max(120 * f0 - 120, 0)
        return wavs[i][base:120 * f1 + 120 if end is None else end], base

    # jobs of 0, 1, 7 and ring_cols columns in one launch
    both([(wavs[0][:1000], 0, 0, 0, 0, -1), (cut(1, 0, 1)[0], 0, 0, 1, 1, -1), (cut(2, 0, 7)[0], 0, 0, 7, 2, -1),
          (cut(3, 0, RING_COLS)[0], 0, 0, RING_COLS, 3, -1)])
    assert bool((arena[0] == SENTINEL).all()) and int((arena[1] != SENTINEL).any(dim=0).sum()) == 1
    assert int((arena[2] != SENTINEL).any(dim=0).sum()) == 7 and torch.equal(arena[3], specs[3][:, :RING_COLS])
    both([(cut(0, 0, 500)[0], 0, 0, 500, 0, -1), (*cut(1, 1, 500), 1, 500, 1, -1), (*cut(2, 7, 500), 7, 500, 2, -1),
          (*cut(3, 512, 520), 512, 520, 3, -1)])
    for i in range(3):
        assert torch.equal(arena[i][:, :500], specs[i][:, :500]) and bool((arena[i][:, 500:] == SENTINEL).all())
    assert torch.equal(arena[3][:, :8], specs[3][:, 512:520]) and torch.equal(arena[3][:, 8:], specs[3][:, 8:512])
    # one job across its ring's wrap, one with n_total >= 0 (the column the end of the signal adds), one without columns
    both([(*cut(0, 500, 530), 500, 530, 0, -1), (*cut(1, 500, 501, end=n_end), 500, 501, 1, n_end), (wavs[2][:0], 0, 500, 500, 2, -1)])
    assert torch.equal(arena[0][:, 500:], specs[0][:, 500:512]) and torch.equal(arena[0][:, :18], specs[0][:, 512:530])
    assert torch.equal(arena[0][:, 18:500], specs[0][:, 18:500])
    assert torch.equal(arena[1][:, 500], offline[:, 500]) and not torch.equal(offline[:, 500], specs[1][:, 500])
    assert bool((arena[2][:, 500:] == SENTINEL).all()) and bool((arena[1][:, 501:] == SENTINEL).all())


def test_group_stft_refuses_before_it_launches(audio):
    wavs = audio["wavs"]
    arena = torch.full((4, 256, RING_COLS), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="two jobs"):
        inputs.group_stft([(wavs[0], 0, 0, 2, 1, -1), (wavs[1], 0, 0, 2, 1, -1)], arena)
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        inputs.group_stft([(wavs[0], 0, 0, 2, 4, -1)], arena)
    with pytest.raises(ValueError, match="the buffer holds"):
        inputs.group_stft([(wavs[0], 0, 0, 2, 0, -1), (wavs[1][:239], 0, 0, 2, 1, -1)], arena)
    with pytest.raises(ValueError, match="one turn"):
        inputs.group_stft([(wavs[0], 0, 0, RING_COLS + 1, 0, -1)], arena)
    assert bool((arena == SENTINEL).all())


def _ring_of(spec, newest):
    """The ring of a stream whose last written column is `newest`: its live columns, the rest NaN."""
    ring = torch.full((256, RING_COLS), float("nan"), dtype=torch.float32, device=DEV)
    live = torch.arange(max(newest - RING_COLS + 1, 0), newest + 1, device=DEV)
    ring[:, live % RING_COLS] = spec[:, live]
    return ring


def test_group_audio_windows_equal_stream_audio_windows_of_each_rows_ring(audio):
    specs = audio["specs"]
    newest = [749, 600, 300]                                      # live columns [238, 749], [89, 600], [0, 300]
    rings = torch.stack([_ring_of(specs[i], newest[i]) for i in range(3)])
    stream_of = [0, 1, 0, 2]                                      # rows alternate between slots whose newest differ
    # 512 in slot 0: across the wrap; 600: inside slot 0's live span, outside slot 1's (columns up to 727 > 600)
    cen = np.array([[512, 600], [300, 600], [400, 621], [128, 172]], dtype=np.int64)
    got = inputs.group_audio_windows(rings, stream_of, newest, cen, check=False)
    assert got.shape == (4, 1, 2, 256, 256)
    for b, i in enumerate(stream_of):
        for t in range(2):
            c = int(cen[b, t])
            if (b, t) == (1, 1):
                assert bool(torch.isnan(got[b, 0, t]).all())
                continue
            one = np.array([[c]], dtype=np.int64)
            want = inputs.stream_audio_windows(rings[i], newest[i], torch.from_numpy(one).to(DEV), one)[0, 0, 0]
            assert torch.equal(got[b, 0, t], want) and torch.equal(want, specs[i][:, c - 128:c + 128]), (b, t)
    assert not torch.equal(got[0, 0, 1], got[2, 0, 1])
    with pytest.raises(ValueError, match="row 1 .stream 1. reaches outside"):
        inputs.group_audio_windows(rings, stream_of, newest, cen)
    ok = cen.copy()
    ok[1, 1] = 472
    assert torch.equal(inputs.group_audio_windows(rings, stream_of, newest, ok)[[0, 2, 3]], got[[0, 2, 3]])
    # a stream_of out of range is NaN on the device and a ValueError on the host; a stream without columns (newest -1) is NaN
    bad = inputs.group_audio_windows(rings, [0, 3, -1, 2], newest, cen, check=False)
    assert torch.equal(bad[[0, 3]], got[[0, 3]]) and bool(torch.isnan(bad[[1, 2]]).all())
    with pytest.raises(ValueError, match="outside"):
        inputs.group_audio_windows(rings, [0, 3, 0, 2], newest, cen)
    none = inputs.group_audio_windows(rings, stream_of, [749, 600, -1], cen, check=False)
    assert bool(torch.isnan(none[3]).all()) and torch.equal(none[[0, 2]], got[[0, 2]])
