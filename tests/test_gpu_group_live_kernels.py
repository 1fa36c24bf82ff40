"""csts_group_live_add and csts_group_live_rows against the single-stream kernels they batch (no model): after any sequence of
group_live_add calls the ring of slot i equals, bit for bit, the ring ops.live_track_add builds from the same calls restricted
to the rows of stream i, and the rows of group_live_rows equal ops.live_track_rows on that ring.  3 streams, 7 ring slots, five
calls whose targets wrap the ring; map sizes that take every path of the kernels: 64 x 64 (the model's), 1 x 1, 3 x 5 (scalar),
40 x 40 (2 chunks a lane) and 64 x 128 (8 chunks, the limit)."""
import itertools
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
STREAMS, RT, FRAMES = 3, 7, 21
SIZES = [(64, 64), (1, 1), (3, 5), (40, 40), (64, 128)]
OUTPUTS = ("heatmaps", "rescaled", "points", "peak", "count", "neighbours")
# (stream of every row, target of every row, live_from of every slot, through ops?)
CALLS = [
    ([0, 1, 2, 0, 1], [0, 1, 2, 3, 5], [0, 0, 0], True),
    ([0, 0, 0, 2, 1], [4, 4, 4, 4, 6], [0, 0, 0], True),                # stream 0: three rows of frame 4 in one call
    ([0, 2, 2, 0], [8, 9, 9, 3], [3, 3, 3], True),                      # no row of stream 1; 8 and 9 recycle, 3 carries on
    ([-1, 3, 1, 0, 2, 1, 0], [10, 10, 10, 12, 13, 10, -1], None, False),  # streams -1 and 3 and a negative target: ignored
    ([0, 1, 2, 2], [15, 17, 16, 20], [9, 11, 14], True),                # slots recycled again
]


def bits(a, b):
    """Exact equality: floats by bit pattern (NaN included), everything else by value."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def raw_add(arena, maps, streams, targets):
    """csts_group_live_add itself, without the host checks of ops.group_live_add."""
    t = torch.tensor(targets, dtype=torch.int64, device=DEV)
    s = torch.tensor(streams, dtype=torch.int32, device=DEV)
    n, rt, h, w = arena["sum"].shape
    rc = lib.load().csts_group_live_add(maps.data_ptr(), t.data_ptr(), s.data_ptr(), len(targets), h, w, arena["sum"].data_ptr(),
                                        arena["count"].data_ptr(), arena["frame"].data_ptr(), n, rt, ops._stream())
    assert rc == 0, lib.load().csts_last_error()
    torch.cuda.synchronize()


def arena_equals_rings(arena, rings):
    for i, ring in enumerate(rings):
        for k in ("sum", "count", "frame"):
            assert bits(arena[k][i], ring[k]), (i, k)


def check_rows(arena, rings, mode, max_gap, want=OUTPUTS, ref=None):
    """Every frame of every stream in one launch, interleaved (frame-major), against live_track_rows ring by ring."""
    stream_of = np.tile(np.arange(STREAMS, dtype=np.int32), FRAMES)
    frame_of = np.repeat(np.arange(FRAMES, dtype=np.int64), STREAMS)
    got = ops.group_live_rows(arena, stream_of, frame_of, mode=mode, max_gap=max_gap, want=want)
    assert sorted(got) == sorted(want)
    ref = ref or [ops.live_track_rows(ring, 0, FRAMES, mode=mode, max_gap=max_gap) for ring in rings]
    for i in range(STREAMS):
        for k in want:
            assert bits(got[k][i::STREAMS], ref[i][k]), (i, k, mode, max_gap)
    return ref


@pytest.mark.parametrize("h,w", SIZES)
def test_arena_and_rows_equal_the_single_stream_kernels(h, w):
    g = torch.Generator().manual_seed(h * 1000 + w)
    arena = ops.group_live_ring(STREAMS, RT, h, w, DEV)
    rings = [ops.live_track_ring(RT, h, w, DEV) for _ in range(STREAMS)]
    assert tuple(arena["sum"].shape) == (STREAMS, RT, h, w) and int(arena["frame"].max()) == -1 and int(arena["count"].sum()) == 0
    seen = set()
    for streams, targets, live_from, through_ops in CALLS:
        maps = torch.rand(len(targets), h, w, generator=g).to(DEV)
        if through_ops:
            ops.group_live_add(maps, torch.tensor(targets, dtype=torch.int64, device=DEV),
                               torch.tensor(streams, dtype=torch.int32, device=DEV), targets, streams, arena, live_from)
        else:
            raw_add(arena, maps, streams, targets)
        for i in range(STREAMS):
            mine = [p for p, (s, t) in enumerate(zip(streams, targets)) if s == i and t >= 0]
            if mine:                                             # a call without a row of stream i is skipped for ring i
                t_i = [targets[p] for p in mine]
                ops.live_track_add(maps[mine], torch.tensor(t_i, dtype=torch.int64, device=DEV), t_i, rings[i],
                                   live_from=max(t_i) - RT + 1)
                seen.add(i)
        arena_equals_rings(arena, rings)
        for mode, max_gap in itertools.product(("hold", "linear"), (3, 9)):
            check_rows(arena, rings, mode, max_gap)
    assert seen == {0, 1, 2}
    assert int(arena["count"][0, 4]) == 3 and int(arena["frame"][0, 4]) == 4          # three rows of one frame, one call
    assert int(arena["count"][0, 3]) == 2 and arena["frame"][0].tolist() == [0, 15, -1, 3, 4, 12, -1]
    assert arena["frame"][1].tolist() == [-1, 1, -1, 17, -1, 5, 6] and int(arena["count"][1, 3]) == 1
    assert arena["frame"][2].tolist() == [-1, -1, 16, -1, 4, -1, 20] and int(arena["count"][2, 2]) == 1
    # every subset of the outputs, on the final state
    ref = check_rows(arena, rings, "linear", 3)
    kinds = set()
    for i in range(STREAMS):
        for c, (a, _) in zip(ref[i]["count"].tolist(), ref[i]["neighbours"].tolist()):
            kinds.add("predicted" if c else "filled" if a >= 0 else "unpredicted")
    assert kinds == {"predicted", "filled", "unpredicted"}
    for r in range(1, len(OUTPUTS)):
        for want in itertools.combinations(OUTPUTS, r):
            check_rows(arena, rings, "linear", 3, want=want, ref=ref)


def test_a_call_without_rows_for_a_ring_leaves_it_untouched_and_refusals_write_nothing():
    h, w = 3, 5
    g = torch.Generator().manual_seed(7)
    arena = ops.group_live_ring(STREAMS, RT, h, w, DEV)
    maps = torch.rand(4, h, w, generator=g).to(DEV)

    def add(streams, targets, live_from=(0, 0, 0), ring=arena, m=maps):
        ops.group_live_add(m, torch.tensor(targets, dtype=torch.int64, device=DEV),
                           torch.tensor(streams, dtype=torch.int32, device=DEV), targets, streams, ring, list(live_from))

    add([0, 2, 2, 0], [1, 2, 3, 1])
    assert int(arena["count"][1].sum()) == 0 and int(arena["frame"][1].max()) == -1 and float(arena["sum"][1].abs().sum()) == 0.0
    before = {k: v.clone() for k, v in arena.items()}
    with pytest.raises(ValueError, match=">= 0"):
        add([0, 1, 2, 0], [4, -1, 5, 6])
    with pytest.raises(ValueError, match="stream 3"):
        add([0, 3, 2, 0], [4, 4, 5, 6])
    with pytest.raises(ValueError, match="stream -1"):
        add([0, -1, 2, 0], [4, 4, 5, 6])
    with pytest.raises(ValueError, match="target 9 of stream 1 would overwrite the slot of frame 2"):
        add([0, 1, 2, 0], [9, 9, 5, 6], live_from=(3, 2, 0))       # 9 < 3 + 7 on stream 0, 9 >= 2 + 7 on stream 1
    with pytest.raises(ValueError, match="one integer per slot"):
        add([0, 1, 2, 0], [4, 4, 5, 6], live_from=(0, 0))
    with pytest.raises(ValueError, match="not a tensor"):
        ops.group_live_add(maps, torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV),
                           torch.zeros(4, dtype=torch.int64), [0] * 4, arena, [0, 0, 0])
    with pytest.raises(ValueError, match="maps must be fp32"):
        add([0, 1, 2, 0], [4, 4, 5, 6], m=maps[:, :, :4])
    with pytest.raises(ValueError, match="frames >= 0"):
        ops.group_live_rows(arena, [0, 1], [3, -1])
    with pytest.raises(ValueError, match="2\\^31"):
        ops.group_live_rows(arena, [0, 1], [3, 2 ** 31 - 9])
    with pytest.raises(ValueError, match="want must name"):
        ops.group_live_rows(arena, [0], [3], want=("overlay",))
    torch.cuda.synchronize()
    for k in arena:
        assert bits(arena[k], before[k]), k
    add([0, 1, 2, 0], [9, 8, 5, 6], live_from=(3, 2, 0))           # the legal neighbour of the refused call goes through
    assert int(arena["frame"][0, 2]) == 9 and int(arena["frame"][1, 1]) == 8


@pytest.mark.parametrize("h,w", [(64, 64), (3, 5)])
def test_rows_of_a_stream_outside_the_arena_are_the_unpredicted_row(h, w):
    g = torch.Generator().manual_seed(11)
    arena = ops.group_live_ring(STREAMS, RT, h, w, DEV)
    t = [2, 2, 2]
    ops.group_live_add(torch.rand(3, h, w, generator=g).to(DEV), torch.tensor(t, dtype=torch.int64, device=DEV),
                       torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV), t, [0, 1, 2], arena, [0, 0, 0])
    got = ops.group_live_rows(arena, [-1, 0, 3, 2, 2 ** 31 - 1, -2 ** 31], [2, 2, 2, 2, 2, 2], mode="hold", max_gap=3)
    for k in (0, 2, 4, 5):
        assert float(got["heatmaps"][k].abs().sum()) == 0.0 and float(got["rescaled"][k].abs().sum()) == 0.0
        assert bool(torch.isnan(got["points"][k]).all()) and float(got["peak"][k]) == 0.0
        assert int(got["count"][k]) == 0 and got["neighbours"][k].tolist() == [-1, -1]
    for k, i in ((1, 0), (3, 2)):
        assert int(got["count"][k]) == 1 and got["neighbours"][k].tolist() == [2, 2]
        assert bits(got["heatmaps"][k], arena["sum"][i, 2])       # a mean of one map: sum * (1 / 1)
