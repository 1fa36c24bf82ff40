"""The sampling passes reading 4:2:0 pictures in place (csts_spatial_sample_yuv, csts_clip_sample_yuv, csts_batch_sample_yuv):
for both layouts the result equals, bit for bit (torch.equal), the RGB pass on inputs.yuv_to_rgb of the pictures -- identity,
downscale, upscale, flip, the three test-mode crops, an odd x0, train parameters under a fixed key, S no multiple of 4; clip
indices outside [0, N - 1] clamp; a batch of three recordings of three sizes at odd byte offsets, the last ending with the arena;
a bad table row gives a NaN clip and leaves the others alone; a captured graph follows a rewritten frames_idx."""
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
FORMATS = ("nv12", "i420")
B, T = 2, 3
COLOUR = {"nv12": dict(matrix="bt601", full_range=False), "i420": dict(matrix="bt709", full_range=True)}


def _yuv(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, device=DEV, dtype=torch.uint8)


def _par(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


TABLES = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]


@pytest.fixture(scope="module")
def pictures():
    """(B, T) 4:2:0 pictures of 50 x 70 and, per layout, their RGB conversion under COLOUR[layout]."""
    frames = _yuv((B, T, 75, 70), 3)
    return frames, {f: inputs.yuv_to_rgb(frames, f, **COLOUR[f]) for f in FORMATS}


def _test_rows(H, W, S):
    """The test-mode rule's rows for crops 0, 1, 2."""
    return [inputs.spatial_rule_host(np.zeros((1, T, 2)), H, W, S, train=False, spatial_idx=k)[0][0].tolist() for k in range(3)]


CASES = {
    "downscale": (32, [[32, 44, 0, 6, 0], [32, 44, 0, 12, 0]]),
    "upscale": (64, [[64, 89, 0, 12, 0], [64, 89, 0, 25, 0]]),
    "flip": (32, [[40, 56, 3, 8, 1], [36, 50, 4, 18, 1]]),
    "odd_x0": (32, [[50, 70, 17, 37, 0], [50, 70, 1, 3, 1]]),                 # unresized: the crop starts at an odd pixel
    "crops_0_1": (32, _test_rows(50, 70, 32)[:2]),
    "crops_2_1": (32, _test_rows(50, 70, 32)[:0:-1]),
    "S_30": (30, [[35, 49, 1, 3, 1], [45, 63, 10, 30, 0]]),                    # S % 4 != 0: the scalar store path
    "S_31_up": (31, [[75, 105, 44, 74, 0], [75, 105, 0, 0, 1]]),
}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_spatial_sample_equals_convert_then_sample(fmt, case, pictures):
    FRAMES, RGB = pictures
    S, rows = CASES[case]
    params = _par(rows)
    got = inputs.spatial_sample(FRAMES, params, S, pixel_format=fmt, **COLOUR[fmt])
    want = inputs.spatial_sample(RGB[fmt], params, S)
    assert got.shape == (B, 3, T, S, S) and got.dtype == torch.float32
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("matrix,full_range", TABLES)
def test_every_layout_under_every_table(fmt, matrix, full_range, pictures):
    """Layout and table are independent: each of the 8 pairs, a resized, flipped crop and an unresized one at an odd x0."""
    frames = pictures[0]
    rgb = inputs.yuv_to_rgb(frames, fmt, matrix, full_range)
    for S, rows in (CASES["flip"], CASES["odd_x0"]):
        params = _par(rows)
        got = inputs.spatial_sample(frames, params, S, pixel_format=fmt, matrix=matrix, full_range=full_range)
        assert torch.equal(got, inputs.spatial_sample(rgb, params, S))
    others = [t for t in TABLES if t != (matrix, full_range)]
    assert all(not torch.equal(rgb, inputs.yuv_to_rgb(frames, fmt, *t)) for t in others)      # the tables do differ on this input


@pytest.mark.parametrize("fmt", FORMATS)
def test_identity_equals_normalize_frames(fmt):
    S = 48
    yuv = _yuv((B, T, 72, 48), 5)
    rgb = inputs.yuv_to_rgb(yuv, fmt, **COLOUR[fmt])
    params = _par([[S, S, 0, 0, 0]] * B)
    got = inputs.spatial_sample(yuv, params, S, pixel_format=fmt, **COLOUR[fmt])
    assert torch.equal(got, inputs.spatial_sample(rgb, params, S))
    assert torch.equal(got, inputs.normalize_frames(rgb))


@pytest.mark.parametrize("fmt", FORMATS)
def test_train_parameters_under_a_fixed_key(fmt, pictures):
    FRAMES, RGB = pictures
    S = 32
    g = torch.Generator().manual_seed(8)
    labels = torch.rand(B, T, 3, generator=g, dtype=torch.float64).to(DEV)
    key = torch.tensor([0x1234_5678_9ABC_DEF1], dtype=torch.int64, device=DEV)
    kw = dict(train=True, min_scale=34, max_scale=48, key=key, return_params=True)
    video, new, params = inputs.spatial_sampling(FRAMES, labels, S, pixel_format=fmt, **COLOUR[fmt], **kw)
    want_v, want_l, want_p = inputs.spatial_sampling(RGB[fmt], labels, S, **kw)
    assert torch.equal(params, want_p) and torch.equal(new, want_l) and torch.equal(video, want_v)
    assert bool((params[:, 0] >= S).all())
    wav = 0.1 * torch.randn(B, 24000 * 5, device=DEV)                         # 5 s: the spectrogram holds an audio window
    idx = (torch.arange(T, device=DEV, dtype=torch.float32) + 0.5)[None].expand(B, T)
    batch = inputs.assemble_batch(FRAMES, wav, idx, float(T), labels, spatial=dict(crop_size=S, train=False), pixel_format=fmt,
                                  **COLOUR[fmt])
    assert torch.equal(batch["video"], inputs.spatial_sampling(RGB[fmt], labels, S, train=False)[0])


@pytest.mark.parametrize("fmt", FORMATS)
def test_bad_params_give_a_nan_clip(fmt, pictures):
    FRAMES, RGB = pictures
    params = _par([[32, 44, 0, 13, 0], [32, 44, 0, 6, 0]])                    # x0 13 > 44 - 32
    got = inputs.spatial_sample(FRAMES, params, 32, pixel_format=fmt, **COLOUR[fmt])
    assert bool(torch.isnan(got[0]).all())
    assert torch.equal(got[1], inputs.spatial_sample(RGB[fmt], params, 32)[1])


@pytest.mark.parametrize("fmt", FORMATS)
def test_clip_sample_clamps_the_indices(fmt):
    S, N = 32, 5
    video = _yuv((N, 75, 70), 9)
    rgb = inputs.yuv_to_rgb(video, fmt, **COLOUR[fmt])
    idx = torch.tensor([[0, 4, 2], [-2, N + 3, 1]], dtype=torch.int32, device=DEV)
    params = _par([[32, 44, 0, 7, 0], [40, 56, 5, 11, 1]])
    got = inputs.clip_sample(video, idx, params, S, pixel_format=fmt, **COLOUR[fmt])
    assert torch.equal(got, inputs.clip_sample(rgb, idx, params, S))
    clamped = torch.tensor([[0, 4, 2], [0, N - 1, 1]], dtype=torch.int32, device=DEV)
    assert torch.equal(got, inputs.clip_sample(video, clamped, params, S, pixel_format=fmt, **COLOUR[fmt]))
    assert torch.equal(got, inputs.spatial_sample(video[clamped.long()], params, S, pixel_format=fmt, **COLOUR[fmt]))


SHAPES = [(5, 34, 50), (3, 40, 36), (7, 36, 52)]                               # N, H, W
IDX = [[0, 4, 4, 2], [2, 1, 0, 1], [-2, 7 + 3, 0, 6]]
PARAMS = [[32, 47, 0, 7, 0], [40, 36, 5, 2, 1], [40, 57, 8, 20, 0]]


def _arena():
    """One pad byte, then the recordings back to back: each starts at an odd byte, the last ends with the arena."""
    recs = [_yuv((n, h * 3 // 2, w), 20 + i) for i, (n, h, w) in enumerate(SHAPES)]
    arena = torch.cat([torch.zeros(1, dtype=torch.uint8, device=DEV)] + [r.reshape(-1) for r in recs])
    offs = 1 + np.cumsum([0] + [r.numel() for r in recs])
    clips = np.array([[offs[i], *SHAPES[i]] for i in range(3)], dtype=np.int64)
    assert all(o % 2 == 1 for o in offs[:3]) and offs[3] == arena.numel() and arena.data_ptr() % 16 == 0
    return recs, arena, clips


def _per_recording(recs, fmt, order, idx, params, S):
    return torch.cat([inputs.clip_sample(inputs.yuv_to_rgb(recs[r], fmt, **COLOUR[fmt]), idx[b:b + 1], params[b:b + 1], S)
                      for b, r in enumerate(order)])


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_sample_of_three_recordings(fmt):
    S = 32
    recs, arena, clips = _arena()
    idx, params = torch.tensor(IDX, dtype=torch.int32, device=DEV), _par(PARAMS)
    tab = torch.from_numpy(clips).to(DEV)
    got = inputs.batch_sample(arena, tab, idx, params, S, clips, pixel_format=fmt, **COLOUR[fmt])
    want = _per_recording(recs, fmt, [0, 1, 2], idx, params, S)
    assert got.shape == (3, 3, 4, S, S) and torch.equal(got, want) and bool(torch.isfinite(got).all())
    # one bad row on the device (the host table vouches for the good one): NaN clip, the others as they were
    for bad_row in ([clips[1, 0], 3, 40, 35], [clips[1, 0], 3, 39, 36], [clips[2, 0], 8, 36, 52], [-16, 3, 40, 36]):
        bad = clips.copy()
        which = 2 if bad_row[1] == 8 else 1
        bad[which] = bad_row
        out = inputs.batch_sample(arena, torch.from_numpy(bad).to(DEV), idx, params, S, clips, pixel_format=fmt, **COLOUR[fmt])
        assert bool(torch.isnan(out[which]).all()), bad_row
        keep = [b for b in range(3) if b != which]
        assert torch.equal(out[keep], want[keep]), bad_row
    with pytest.raises(ValueError):                                           # the wrapper refuses such a table on the host
        bad = clips.copy()
        bad[2, 1] = 8
        inputs.batch_sample(arena, tab, idx, params, S, bad, pixel_format=fmt, **COLOUR[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_graph_follows_the_rewritten_indices(fmt):
    S = 32
    recs, arena, clips = _arena()
    idx, params = torch.tensor(IDX, dtype=torch.int32, device=DEV), _par(PARAMS)
    tab = torch.from_numpy(clips).to(DEV)
    out = torch.empty(3, 3, 4, S, S, dtype=torch.float32, device=DEV)

    def step():
        return inputs.batch_sample(arena, tab, idx, params, S, clips, out=out, pixel_format=fmt, **COLOUR[fmt])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = step().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()                                                                # no host sync inside: the capture would fail on one
    idx.copy_(torch.tensor([[4, 3, 2, 1], [1, 1, 9, -1], [6, 0, 1, 1]], dtype=torch.int32, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = inputs.batch_sample(arena, tab, idx, params, S, clips, pixel_format=fmt, **COLOUR[fmt])
    assert torch.equal(replayed, eager) and not torch.equal(replayed, first)
    assert torch.equal(eager, _per_recording(recs, fmt, [0, 1, 2], idx, params, S))
