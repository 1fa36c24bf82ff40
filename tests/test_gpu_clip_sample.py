"""csts_clip_sample (csts_amd/csrc/spatial.hip, inputs.clip_sample): sampling clips straight out of a resident video equals,
bit for bit, gathering the frames first and running spatial_sample -- with repeated, descending and out-of-range (clamped)
indices, frame strides that leave every frame base at another misalignment, per-clip crops and a flip, and identity
parameters (= normalize_frames); the index table is read on the device, so a captured graph resamples after the table is
rewritten in place."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import inputs, lib  # noqa: E402

DEV = torch.device("cuda:0")
N, B, T = 7, 3, 4
# repeats, descending order, 0, N - 1 and out-of-range values on both sides
TABLE = [[0, 6, 6, 3], [5, 4, 2, 1], [-2, N + 3, 0, 6]]


def _video(H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, (N, H, W, 3), generator=g, device=DEV, dtype=torch.uint8)


def _table(rows=TABLE):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def _gathered(video, idx):
    return video[idx.long().clamp(0, video.shape[0] - 1)]            # (B, T, H, W, 3), the clamp of temporal_sampling


def test_misaligned_frame_bases_35x51():
    """35 * 51 * 3 = 5355 bytes a frame, not a multiple of 16: every frame starts at another offset inside a 16-byte chunk."""
    video = _video(35, 51, 1)
    assert (35 * 51 * 3) % 16 != 0 and len({(i * 5355) % 16 for i in range(N)}) == N
    idx = _table()
    params = torch.tensor([[32, 46, 0, 7, 0]] * B, dtype=torch.int32, device=DEV)       # short side 35 -> 32, centre crop
    got = inputs.clip_sample(video, idx, params, 32)
    want = inputs.spatial_sample(_gathered(video, idx), params, 32)
    assert got.shape == (B, 3, T, 32, 32) and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert bool(torch.isfinite(got).all())
    # the clamp: -2 reads frame 0, N + 3 reads frame N - 1
    assert torch.equal(got[2, :, 0], got[0, :, 0]) and torch.equal(got[2, :, 1], got[0, :, 1])


def test_flip_and_distinct_crops_36x52():
    video = _video(36, 52, 2)
    idx = _table()
    params = torch.tensor([[36, 52, 2, 11, 0], [40, 57, 8, 20, 1], [32, 46, 0, 14, 0]], dtype=torch.int32, device=DEV)
    got = inputs.clip_sample(video, idx, params, 32)
    assert torch.equal(got, inputs.spatial_sample(_gathered(video, idx), params, 32))
    # a crop size that is no multiple of 4 (scalar stores) and more than one row block
    params = torch.tensor([[36, 52, 1, 3, 1], [36, 52, 5, 20, 0], [45, 65, 10, 30, 0]], dtype=torch.int32, device=DEV)
    got = inputs.clip_sample(video, idx, params, 30)
    assert torch.equal(got, inputs.spatial_sample(_gathered(video, idx), params, 30))


def test_identity_params_equal_normalize_frames():
    video = _video(32, 32, 3)
    idx = _table()
    params = torch.tensor([[32, 32, 0, 0, 0]] * B, dtype=torch.int32, device=DEV)
    got = inputs.clip_sample(video, idx, params, 32)
    clip = _gathered(video, idx)
    assert torch.equal(got, inputs.spatial_sample(clip, params, 32))
    assert torch.equal(got, inputs.normalize_frames(clip))


def test_graph_replay_reads_the_rewritten_table():
    video = _video(35, 51, 4)
    idx = _table()
    params = torch.tensor([[32, 46, 0, 7, 0]] * B, dtype=torch.int32, device=DEV)
    first = inputs.clip_sample(video, idx, params, 32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        inputs.clip_sample(video, idx, params, 32)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = inputs.clip_sample(video, idx, params, 32)           # no host sync inside: the capture would fail on one
    other = _table([[6, 5, 4, 3], [1, 1, 9, -1], [2, 0, 3, 3]])
    idx.copy_(other)                                               # in place: the graph holds the table's address
    graph.replay()
    torch.cuda.synchronize()
    want = inputs.spatial_sample(_gathered(video, other), params, 32)
    assert torch.equal(out, want) and not torch.equal(out, first)


def test_arguments_are_validated():
    video = _video(36, 52, 5)
    idx = _table()
    params = torch.tensor([[36, 52, 2, 11, 0]] * B, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        inputs.clip_sample(video, idx.long(), params, 32)          # the table is int32
    with pytest.raises(ValueError):
        inputs.clip_sample(video[None], idx, params, 32)           # (N, H, W, 3), not a batch of clips
    with pytest.raises(ValueError):
        inputs.clip_sample(video, idx, params[:2], 32)
    with pytest.raises(ValueError):
        inputs.clip_sample(video, torch.zeros(1, 65, dtype=torch.int32, device=DEV), params[:1], 32)
    with pytest.raises(lib.CstsError):
        inputs.clip_sample(video.cpu(), idx, params, 32)
    # params outside the rule's range give a NaN clip and read nothing, as in spatial_sample
    bad = params.clone()
    bad[1] = torch.tensor([36, 52, 9, 11, 0], dtype=torch.int32)
    out = inputs.clip_sample(video, idx, bad, 32)
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all())
