"""csts_amd/csrc/batch.hip (inputs.batch_sample, batch_params, audio_gather): one launch assembles clips of several recordings of
several sizes, bit for bit what the single-recording ops give per clip.  Three recordings (5, 35, 51), (3, 40, 36), (7, 36, 52)
lie back to back in one arena, so the second and third start at odd bytes; the tables are read on the device, so one captured
graph assembles another batch after they are rewritten in place; a table row that leaves the declared arena gives a NaN clip."""
import ctypes as C
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

from csts_amd import inputs, lib  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(5, 35, 51), (3, 40, 36), (7, 36, 52)]
T = 4
IDX = [[0, 4, 4, 2], [2, 1, 0, 1], [-2, 7 + 3, 0, 6]]          # -2 and N + 3: the clamp
PARAMS = {32: [[32, 46, 0, 7, 0], [40, 36, 5, 2, 1], [40, 57, 8, 20, 0]],         # distinct crops, clip 1 flipped
          30: [[35, 51, 1, 3, 1], [40, 36, 5, 6, 0], [45, 65, 10, 30, 0]]}        # S % 4 != 0: the scalar store path


def _recordings():
    g = torch.Generator(device=DEV).manual_seed(11)
    return [torch.randint(0, 256, (n, h, w, 3), generator=g, device=DEV, dtype=torch.uint8) for n, h, w in SHAPES]


RECS = _recordings()
ARENA = torch.cat([r.reshape(-1) for r in RECS])
OFFS = np.cumsum([0] + [r.numel() for r in RECS])[:3]
CLIPS = np.array([[OFFS[i], *SHAPES[i]] for i in range(3)], dtype=np.int64)


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _per_recording(order, idx, params, S):
    return torch.cat([inputs.clip_sample(RECS[r], idx[b:b + 1], params[b:b + 1], S) for b, r in enumerate(order)])


def test_recordings_start_at_odd_bytes():
    assert OFFS[1] % 2 == 1 and OFFS[2] % 2 == 1 and ARENA.data_ptr() % 16 == 0


@pytest.mark.parametrize("S", [32, 30])
def test_batch_sample_equals_clip_sample_per_recording(S):
    idx, params = _dev(IDX, torch.int32), _dev(PARAMS[S], torch.int32)
    got = inputs.batch_sample(ARENA, _dev(CLIPS, torch.int64), idx, params, S, CLIPS)
    want = _per_recording([0, 1, 2], idx, params, S)
    assert got.shape == (3, 3, T, S, S) and got.dtype == torch.float32
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    # the clamp: frame -2 is frame 0 and frame N + 3 is frame N - 1 of recording 2
    assert torch.equal(got[2, :, 0], got[2, :, 2]) and torch.equal(got[2, :, 1], got[2, :, 3])
    # another order, one recording twice
    order = [2, 0, 2]
    got = inputs.batch_sample(ARENA, _dev(CLIPS[order], torch.int64), idx, params[[2, 0, 2]], S, CLIPS[order])
    assert torch.equal(got, _per_recording(order, idx, params[[2, 0, 2]], S))


@pytest.mark.parametrize("S", [32, 30])
def test_batch_sample_of_one_recording_equals_one_clip_sample(S):
    idx = _dev([[0, 6, 6, 3], [5, 4, 2, 1], [-2, 10, 0, 6]], torch.int32)
    params = _dev([PARAMS[S][2]] * 2 + [[36, 52, 2, 11, 1]], torch.int32)
    tab = CLIPS[[2, 2, 2]]
    got = inputs.batch_sample(ARENA, _dev(tab, torch.int64), idx, params, S, tab)
    assert torch.equal(got, inputs.clip_sample(RECS[2], idx, params, S))


def _raw_sample(clips, arena_bytes, max_W, S=32):
    """csts_batch_sample through the C ABI, past the wrapper's host check."""
    idx, params, tab = _dev(IDX, torch.int32), _dev(PARAMS[S], torch.int32), _dev(clips, torch.int64)
    out = torch.zeros(3, 3, T, S, S, dtype=torch.float32, device=DEV)
    f3 = C.c_float * 3
    lib.check(lib.load().csts_batch_sample(ARENA.data_ptr(), int(arena_bytes), tab.data_ptr(), idx.data_ptr(), params.data_ptr(),
                                           out.data_ptr(), 3, T, S, int(max_W), f3(0.45, 0.45, 0.45), f3(0.225, 0.225, 0.225),
                                           torch.cuda.current_stream().cuda_stream), "csts_batch_sample")
    torch.cuda.synchronize()
    return out


def test_guard_gives_a_nan_clip_and_reads_nothing_outside():
    full = _raw_sample(CLIPS, ARENA.numel(), 52)
    assert torch.equal(full, _per_recording([0, 1, 2], _dev(IDX, torch.int32), _dev(PARAMS[32], torch.int32), 32))
    # the declared arena ends one byte before recording 2 does (the allocation is the full one: nothing unmapped is in reach)
    short = _raw_sample(CLIPS, ARENA.numel() - 1, 52)
    assert bool(torch.isnan(short[2]).all()) and torch.equal(short[:2], full[:2])
    # the declared arena ends inside recording 1
    short = _raw_sample(CLIPS, OFFS[2] - 100, 52)
    assert bool(torch.isnan(short[1:]).all()) and torch.equal(short[0], full[0])
    # rows wider than the staged LDS (W 52 > max_W 51), without frames, with a negative offset
    out = _raw_sample(CLIPS, ARENA.numel(), 51)
    assert bool(torch.isnan(out[2]).all()) and torch.equal(out[:2], full[:2])
    bad = CLIPS.copy()
    bad[0, 1] = 0
    bad[1, 0] = -16
    out = _raw_sample(bad, ARENA.numel(), 52)
    assert bool(torch.isnan(out[:2]).all()) and torch.equal(out[2], full[2])
    # the wrapper refuses such a table on the host
    with pytest.raises(ValueError):
        inputs.batch_sample(ARENA[:-16], _dev(CLIPS, torch.int64), _dev(IDX, torch.int32), _dev(PARAMS[32], torch.int32), 32, CLIPS)
    with pytest.raises(ValueError):
        inputs.batch_sample(ARENA, _dev(bad, torch.int64), _dev(IDX, torch.int32), _dev(PARAMS[32], torch.int32), 32, bad)
    with pytest.raises(ValueError):
        inputs.batch_sample(ARENA, _dev(CLIPS, torch.int32), _dev(IDX, torch.int32), _dev(PARAMS[32], torch.int32), 32, CLIPS)


def _labels(B, seed):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(B, T, 2, generator=g, dtype=torch.float64)
    return torch.cat([xy, torch.randint(0, 2, (B, T, 1), generator=g).double()], dim=-1).to(DEV)


KEY = 0x1234_5678_9ABC_DEF1
TRAIN = dict(train=True, min_scale=32, max_scale=48, random_flip=True, inverse_uniform=False)


@pytest.mark.parametrize("train", [True, False])
def test_batch_params_with_equal_sizes_equals_spatial_params(train):
    B, H, W, S = 5, 36, 52, 32
    labels = _labels(B, 3)
    tab = np.tile(np.array([[0, 7, H, W]], dtype=np.int64), (B, 1))
    key = torch.tensor([KEY], dtype=torch.int64, device=DEV)
    kw = TRAIN if train else dict(train=False, spatial_idx=2)
    params, new = inputs.batch_params(labels, _dev(tab, torch.int64), S, key=key, clips_host=tab, **kw)
    want_p = torch.empty(B, 5, dtype=torch.int32, device=DEV)
    want_l = torch.empty_like(labels)
    lib.check(lib.load().csts_spatial_params(key.data_ptr(), labels.data_ptr(), B, T, 3, H, W, S, kw.get("min_scale", 0),
                                             kw.get("max_scale", 0), -1 if train else 2, 1, 0, want_p.data_ptr(), want_l.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "csts_spatial_params")
    assert torch.equal(params, want_p) and torch.equal(new, want_l)
    assert bool((params[:, 0] >= S).all())


@pytest.mark.parametrize("train", [True, False])
def test_batch_params_with_mixed_sizes_equals_the_host_rule_per_clip(train):
    S = 32
    order = [0, 1, 2, 1, 0]
    labels = _labels(len(order), 4)
    tab = CLIPS[order]
    key = torch.tensor([KEY], dtype=torch.int64, device=DEV)
    kw = TRAIN if train else dict(train=False, spatial_idx=1)
    params, new = inputs.batch_params(labels, _dev(tab, torch.int64), S, key=key, clips_host=tab, **kw)
    lab = labels.cpu().numpy()
    for b, r in enumerate(order):
        _, H, W = SHAPES[r]
        u = inputs.spatial_uniforms_host(KEY, b, 1) if train else None            # clip b draws u[b]
        want_p, want_l = inputs.spatial_rule_host(lab[b:b + 1], H, W, S, uniforms=u, **kw)
        assert np.array_equal(params[b].cpu().numpy(), want_p[0]) and np.array_equal(new[b].cpu().numpy(), want_l[0])
    if train:
        assert len({tuple(p) for p in params.cpu().tolist()}) > 1
    with pytest.raises(ValueError):
        bad = tab.copy()
        bad[1, 2] = 0
        inputs.batch_params(labels, _dev(bad, torch.int64), S, key=key, clips_host=bad, **kw)


NBINS, WIDTH = 8, 16
SPEC_COLS, USABLE = [40, 57, 33], [31, 45, 25]


def _specs():
    g = torch.Generator(device=DEV).manual_seed(5)
    specs = [torch.randn(NBINS, c, generator=g, device=DEV) for c in SPEC_COLS]
    offs = np.cumsum([0] + [s.numel() for s in specs])[:3]
    table = np.array([[offs[i], SPEC_COLS[i], USABLE[i]] for i in range(3)], dtype=np.int64)
    return specs, torch.cat([s.reshape(-1) for s in specs]), table


CENTERS = [[-5, 8, 15, 100], [0, 20, 36, 37], [3, 12, 16, 17]]         # below, inside and above [8, usable - 1 - 8]


def test_audio_gather_equals_audio_windows_at_per_clip():
    specs, arena, table = _specs()
    cen = _dev(CENTERS, torch.int32)
    got = inputs.audio_gather(arena, _dev(table, torch.int64), cen, NBINS, table, WIDTH)
    assert got.shape == (3, 1, T, NBINS, WIDTH)
    for b in range(3):
        want = inputs.audio_windows_at(specs[b][:, :USABLE[b]].contiguous(), cen[b:b + 1], WIDTH)
        assert torch.equal(got[b:b + 1], want)
    order = [2, 0, 2]
    got = inputs.audio_gather(arena, _dev(table[order], torch.int64), cen, NBINS, table[order], WIDTH)
    for b, r in enumerate(order):
        assert torch.equal(got[b:b + 1], inputs.audio_windows_at(specs[r][:, :USABLE[r]].contiguous(), cen[b:b + 1], WIDTH))
    with pytest.raises(ValueError):
        bad = table.copy()
        bad[2, 1] = 64                                                    # the last spectrogram would leave the arena
        inputs.audio_gather(arena, _dev(bad, torch.int64), cen, NBINS, bad, WIDTH)
    with pytest.raises(ValueError):
        bad = table.copy()
        bad[0, 2] = 16                                                    # no window of 16 + 1 columns fits
        inputs.audio_gather(arena, _dev(bad, torch.int64), cen, NBINS, bad, WIDTH)


def test_one_graph_assembles_the_batch_of_the_rewritten_tables():
    S = 32
    specs, sarena, stable = _specs()
    labels = _labels(3, 6)
    key = torch.tensor([KEY], dtype=torch.int64, device=DEV)
    clips, idx = _dev(CLIPS, torch.int64), _dev(IDX, torch.int32)
    spt, cen = _dev(stable, torch.int64), _dev(CENTERS, torch.int32)

    def step():
        params, new = inputs.batch_params(labels, clips, S, key=key, clips_host=CLIPS, **TRAIN)
        return (params, new, inputs.batch_sample(ARENA, clips, idx, params, S, CLIPS),
                inputs.audio_gather(sarena, spt, cen, NBINS, stable, WIDTH))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()                                                      # no host sync inside: the capture would fail on one
    order = [2, 0, 1]
    clips.copy_(_dev(CLIPS[order], torch.int64))                          # in place: the graph holds the tables' addresses
    idx.copy_(_dev([[6, 5, 4, 3], [1, 1, 9, -1], [2, 0, 1, 1]], torch.int32))
    spt.copy_(_dev(stable[order], torch.int64))
    cen.copy_(_dev([[9, 9, 30, 2], [14, 0, 22, 8], [40, 41, 8, 9]], torch.int32))
    key.fill_(KEY + 1)
    graph.replay()
    torch.cuda.synchronize()
    params, new = inputs.batch_params(labels, clips, S, key=key, clips_host=CLIPS[order], **TRAIN)
    assert torch.equal(out[0], params) and torch.equal(out[1], new)
    assert torch.equal(out[2], _per_recording(order, idx, params, S)) and not torch.equal(out[2], first[2])
    for b, r in enumerate(order):
        assert torch.equal(out[3][b:b + 1], inputs.audio_windows_at(specs[r][:, :USABLE[r]].contiguous(), cen[b:b + 1], WIDTH))
