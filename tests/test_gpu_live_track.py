"""The two live-track kernels alone (no model): ops.live_track_add folds window maps into a ring of per-frame sums,
ops.live_track_rows reads track rows out of it.  Pinned bit for bit against the offline pair ops.gaze_track + ops.gaze_track_fill
on the windows added so far: both sides run the same additions in the same order and the same device functions, so every
comparison is exact (floats are compared by their bit patterns, which also pins the NaN points of unpredicted frames)."""
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

from csts_amd import lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
SIZES = [(64, 64), (1, 1), (3, 5)]        # the model's map; the smallest map gaze_track accepts; an odd one (scalar accesses)
T, SPACING, FIRST, SPAN = 8, 9, 86, 64    # a window at origin o targets o + 86 + 9 i, and is ready when frame o + 85 is in
FLOATS = ("heatmaps", "rescaled", "points", "peak")


def bits(a, b):
    """Exact equality: floats by bit pattern (NaN included), everything else by value."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def random_maps(P, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(P, h, w, generator=g, dtype=torch.float32)
    return (m / m.sum(dim=(1, 2), keepdim=True)).to(DEV)


def window_targets(w, stride, local=None):
    local = FIRST + SPACING * np.arange(T, dtype=np.int64) if local is None else np.asarray(local, dtype=np.int64)
    return w * stride + local


def offline(maps, targets, n_frames, mode, max_gap):
    """gaze_track + gaze_track_fill of the maps so far: the outputs a live row has, (n_frames, ...) each."""
    track = ops.gaze_track(maps, torch.from_numpy(targets).to(DEV), n_frames, want=("heatmaps", "count"))
    out = ops.gaze_track_fill(track["heatmaps"], track["count"], mode=mode, max_gap=max_gap)
    out["count"] = track["count"]
    return out


@pytest.fixture(scope="module")
def maps40():
    return {hw: random_maps(40 * T, *hw, seed=7 + i) for i, hw in enumerate(SIZES)}


@pytest.mark.parametrize("per_call", [1, 2, 5])
@pytest.mark.parametrize("mode, max_gap", [("hold", 9), ("linear", 9), ("hold", 4), ("linear", 4), ("hold", 18), ("linear", 18)])
def test_ring_rows_equal_the_offline_track_of_the_windows_so_far(maps40, mode, max_gap, per_call):
    stride, windows = 9, 40
    chunk = stride * per_call                                   # frames that arrive between two calls
    Rt = SPAN + chunk + max_gap - 1                             # the bound of stream.live_ring_slots for this schedule
    assert (windows - 1) * stride + FIRST + SPACING * (T - 1) > 3 * Rt     # the ring turns more than three times
    for hw in SIZES:
        maps = maps40[hw]
        targets = np.concatenate([window_targets(w, stride) for w in range(windows)])
        ring = ops.live_track_ring(Rt, *hw, DEV)
        seen = {"predicted": 0, "filled": 0, "unpredicted": 0}
        for w0 in range(0, windows, per_call):
            w1 = min(w0 + per_call, windows)
            F = (w1 - 1) * stride + FIRST                       # frames in when the call's last window became ready
            f0 = F - chunk
            sel = slice(w0 * T, w1 * T)
            ops.live_track_add(maps[sel], torch.from_numpy(targets[sel]).to(DEV), targets[sel], ring,
                               live_from=max(0, f0 - max_gap + 1))
            got = ops.live_track_rows(ring, f0, chunk, mode=mode, max_gap=max_gap)
            want = offline(maps[:w1 * T], targets[:w1 * T], F - 1 + max_gap + 1, mode, max_gap)
            for k in FLOATS + ("count", "neighbours"):
                assert bits(got[k], want[k][f0:F]), (hw, w0, k)
            # `want` is one track of F - 1 + max_gap + 1 frames, the size the rule gives the call's LAST row.  For an earlier row f
            # the rule's track is shorter, f + max_gap + 1 frames, and has the same row f: the fill of row f looks for a in
            # [f - max_gap + 1, f) and b in (f, a + max_gap], so it reads nothing past frame f + max_gap - 1.  The rule as it is
            # stated is checked on the first row of the call, where the two sizes differ most.
            exact = offline(maps[:w1 * T], targets[:w1 * T], f0 + max_gap + 1, mode, max_gap)
            for k in FLOATS + ("count", "neighbours"):
                assert bits(got[k][:1], exact[k][f0:f0 + 1]), (hw, w0, k, "n_frames = f + max_gap + 1")
            seen["predicted"] += int((got["count"] > 0).sum())
            seen["filled"] += int(((got["count"] == 0) & (got["neighbours"][:, 0] >= 0)).sum())
            seen["unpredicted"] += int((got["neighbours"][:, 0] < 0).sum())
        assert seen["predicted"] > 0 and seen["unpredicted"] > 0, seen
        assert (seen["filled"] > 0) == (max_gap >= SPACING), seen           # max_gap 4 bridges nothing


@pytest.mark.parametrize("hw", SIZES)
def test_several_maps_of_one_call_on_one_slot_add_in_gaze_track_order(hw):
    # stride 9, 12 windows in ONE call: a frame is targeted by up to 8 of them
    maps = random_maps(12 * T, *hw, seed=21)
    targets = np.concatenate([window_targets(w, 9) for w in range(12)])
    n = int(targets.max()) + 12
    want = ops.gaze_track(maps, torch.from_numpy(targets).to(DEV), n)
    assert int(want["count"].max()) == 8
    ring = ops.live_track_ring(n, *hw, DEV)
    ops.live_track_add(maps, torch.from_numpy(targets).to(DEV), targets, ring)
    got = ops.live_track_rows(ring, 0, n, mode="hold", max_gap=1)          # max_gap 1 fills nothing: the sparse track
    for k in FLOATS + ("count",):
        assert bits(got[k], want[k]), k
    # a frame no window targets (inside the span) and the frames past the last prediction: the unpredicted row
    empty = got["count"] == 0
    assert bool(empty[FIRST + 1]) and bool(empty[int(targets.max()) + 1:].all()) and not bool(empty[int(targets.max())])
    assert torch.equal(got["neighbours"][empty], torch.full((int(empty.sum()), 2), -1, dtype=torch.int32, device=DEV))
    assert bool(torch.isnan(got["points"][empty]).all()) and bool((got["peak"][empty] == 0).all())
    assert bool((got["heatmaps"][empty] == 0).all()) and bool((got["rescaled"][empty] == 0).all())
    full = torch.arange(n, device=DEV, dtype=torch.int32)[~empty]
    assert torch.equal(got["neighbours"][~empty], torch.stack([full, full], dim=-1))
    # stride 3 with a target named twice inside one window, fed in two calls: (0 + a) + b ... in ascending p, across the calls
    local = [10, 13, 13, 16, 19, 19, 22, 25]
    maps = random_maps(10 * T, *hw, seed=22)
    targets = np.concatenate([window_targets(w, 3, local) for w in range(10)])
    n = int(targets.max()) + 3
    want = ops.gaze_track(maps, torch.from_numpy(targets).to(DEV), n)
    assert int(want["count"].max()) >= 8
    ring = ops.live_track_ring(n, *hw, DEV)
    for sel in (slice(0, 4 * T), slice(4 * T, 10 * T)):
        ops.live_track_add(maps[sel], torch.from_numpy(targets[sel]).to(DEV), targets[sel], ring)
    got = ops.live_track_rows(ring, 0, n, mode="linear", max_gap=1)
    for k in FLOATS + ("count",):
        assert bits(got[k], want[k]), k


def test_a_recycled_slot_is_empty_for_the_frame_it_held():
    hw, Rt = (64, 64), 16
    maps = random_maps(3, *hw, seed=31)
    ring = ops.live_track_ring(Rt, *hw, DEV)
    t = np.array([5, 7], dtype=np.int64)
    ops.live_track_add(maps[:2], torch.from_numpy(t).to(DEV), t, ring)
    before = ops.live_track_rows(ring, 4, 5, mode="hold", max_gap=4)       # frames 4..8: 5 and 7 predicted, 6 held from 5
    assert before["count"].tolist() == [0, 1, 0, 1, 0] and before["neighbours"].tolist() == [[-1, -1], [5, 5], [5, 7], [7, 7], [-1, -1]]
    assert bits(before["heatmaps"][2], before["heatmaps"][1])
    t2 = np.array([21], dtype=np.int64)                                    # 21 = 5 + Rt: frame 5's slot, once frame 5 is behind
    ops.live_track_add(maps[2:], torch.from_numpy(t2).to(DEV), t2, ring, live_from=6)
    assert ring["frame"][5].item() == 21 and ring["count"][5].item() == 1 and bits(ring["sum"][5], maps[2])
    after = ops.live_track_rows(ring, 4, 5, mode="hold", max_gap=4)        # frame 5 now reads a slot tagged 21: empty
    assert after["count"].tolist() == [0, 0, 0, 1, 0] and after["neighbours"].tolist() == [[-1, -1]] * 3 + [[7, 7], [-1, -1]]
    assert bool(torch.isnan(after["points"][1]).all()) and after["peak"][1].item() == 0 and bool((after["rescaled"][1] == 0).all())
    new = ops.live_track_rows(ring, 21, 1, mode="hold", max_gap=4)
    want = ops.gaze_track(maps[2:], torch.tensor([0], device=DEV), 1)
    for k in FLOATS + ("count",):
        assert bits(new[k], want[k]), k


def test_refusals_leave_the_ring_untouched():
    hw, Rt = (64, 64), 32
    maps = random_maps(4, *hw, seed=41)
    host = np.array([3, 4, 5, 6], dtype=np.int64)
    dev = torch.from_numpy(host).to(DEV)
    ring = ops.live_track_ring(Rt, *hw, DEV)
    ops.live_track_add(maps, dev, host, ring)
    saved = {k: v.clone() for k, v in ring.items()}
    bad = [
        (lambda: ops.live_track_add(maps.double(), dev, host, ring), ValueError, "fp32"),
        (lambda: ops.live_track_add(maps[:, :32], dev, host, ring), ValueError, "fp32"),
        (lambda: ops.live_track_add(maps, dev.int(), host, ring), ValueError, "int64"),
        (lambda: ops.live_track_add(maps, dev[:3], host, ring), ValueError, "int64"),
        (lambda: ops.live_track_add(maps, dev, host[:3], ring), ValueError, "on the host"),
        (lambda: ops.live_track_add(maps, dev, dev, ring), ValueError, "host copy"),
        (lambda: ops.live_track_add(maps, dev, host - 4, ring), ValueError, ">= 0"),
        (lambda: ops.live_track_add(maps.cpu(), dev, host, ring), lib.CstsError, "GPU"),
        (lambda: ops.live_track_add(maps, dev.cpu(), host, ring), lib.CstsError, "GPU"),
        (lambda: ops.live_track_add(maps, dev, host, dict(ring, sum=ring["sum"].cpu())), lib.CstsError, "GPU"),
        (lambda: ops.live_track_add(maps, dev, host, dict(ring, count=ring["count"].long())), ValueError, "int32"),
        (lambda: ops.live_track_add(maps, dev, host, dict(ring, frame=ring["frame"][:-1])), ValueError, "int64"),
        (lambda: ops.live_track_add(maps, dev, host, {"sum": ring["sum"]}), ValueError, "ops.live_track_ring"),
        # frame 3 is still inside the live span: 3 + Rt would take its slot
        (lambda: ops.live_track_add(maps, dev + Rt, host + Rt, ring, live_from=3), ValueError, "would overwrite the slot of frame 6"),
        (lambda: ops.live_track_rows(ring, 0, 0), ValueError, "1..65535"),
        (lambda: ops.live_track_rows(ring, -1, 4), ValueError, "f0 >= 0"),
        (lambda: ops.live_track_rows(ring, 0, 4, mode="nearest"), ValueError, "mode"),
        (lambda: ops.live_track_rows(ring, 0, 4, max_gap=0), ValueError, "max_gap"),
        (lambda: ops.live_track_rows(ring, 0, 4, want=("points", "filled")), ValueError, "want"),
        (lambda: ops.live_track_rows(dict(ring, sum=ring["sum"].cpu()), 0, 4), lib.CstsError, "GPU"),
    ]
    for call, error, word in bad:
        with pytest.raises(error, match=word):
            call()
        for k in saved:
            assert torch.equal(ring[k], saved[k]), (word, k)
    ops.live_track_add(maps, dev + Rt, host + Rt, ring, live_from=7)       # the same targets once frames 3..6 are behind
    assert ring["frame"][3:7].tolist() == (host + Rt).tolist()


@pytest.mark.parametrize("hw", SIZES)
def test_want_subsets_keep_their_bits(hw):
    maps = random_maps(3 * T, *hw, seed=51)
    targets = np.concatenate([window_targets(w, 9) for w in range(3)])
    ring = ops.live_track_ring(200, *hw, DEV)
    ops.live_track_add(maps, torch.from_numpy(targets).to(DEV), targets, ring)
    saved = {k: v.clone() for k, v in ring.items()}
    full = ops.live_track_rows(ring, 80, 90, mode="linear", max_gap=9)
    assert sorted(full) == sorted(FLOATS + ("count", "neighbours"))
    for want in (("points",), ("count", "neighbours"), ("rescaled", "peak"), ("heatmaps",), ("points", "peak", "count", "neighbours")):
        part = ops.live_track_rows(ring, 80, 90, mode="linear", max_gap=9, want=want)
        assert sorted(part) == sorted(want)
        for k in want:
            assert bits(part[k], full[k]), (want, k)
    for k in saved:                                                        # rows only read the ring
        assert torch.equal(ring[k], saved[k]), k
