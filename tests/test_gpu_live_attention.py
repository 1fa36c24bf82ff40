"""The two live-attention kernels alone (no model): ops.live_attention_add folds the audio attention of newly run windows into a
ring of per-frame sums, ops.live_attention_rows answers frames with the newest map at most max_age old.  Pinned bit for bit
against the existing ops: ops.attention_track over everything added so far, a pick of the frame on the host, and
ops.attention_rescale of the picked map.  Both sides run the same additions in the same order and the same device functions, so
every comparison is exact; floats are compared by their bit patterns, which also pins the NaN range of an empty row and the
sign of a zero.  apa_pair_cell CAN produce a negative zero (fl(w0 * -0) + fl(w1 * -0) = -0 for a head whose cell is -0 in both
coarse maps), so one case feeds such a column: the restart must give the bits of 0.f + x = +0, as ops.attention_track's sum does."""
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
S = 32
# heads, T', T, h, w, the frames of a window relative to its origin (ascending; the second names two frames twice)
SHAPES = {"scalar": (2, 2, 4, 3, 5, [0, 1, 2, 4]), "vector": (3, 4, 8, 8, 8, [0, 1, 1, 2, 3, 4, 4, 5])}
ROW_KEYS = ("frame", "count", "mixed", "maps", "range")


def bits(a, b):
    """Exact equality: floats by bit pattern (NaN and the sign of zero included), everything else by value."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def columns(n, shape, seed):
    heads, Tp, _, h, w, _ = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, heads, Tp, h, w, generator=g, dtype=torch.float32).to(DEV)


def window_frames(shape, origins):
    return np.stack([o + np.asarray(SHAPES[shape][5], dtype=np.int64) for o in origins])


def add(ring, column, frames, live_from=0):
    ops.live_attention_add(column, torch.from_numpy(frames).to(DEV), frames, ring, live_from=live_from)


def offline(column, frames, f0, K, T, max_age):
    """The rule on the existing ops: attention_track of everything added, the pick on the host, attention_rescale of the pick."""
    A = ops.attention_track(column, torch.from_numpy(frames).to(DEV), f0 + K, T, S)
    count = A["count"].cpu().numpy()
    pick = [next((g for g in range(n, max(0, n - max_age) - 1, -1) if count[g] > 0), -1) for n in range(f0, f0 + K)]
    frame = torch.tensor(pick, dtype=torch.int64, device=DEV)
    have, at = frame >= 0, frame.clamp(min=0)
    mixed = torch.where(have[:, None, None, None], A["mixed"][at], torch.zeros_like(A["mixed"][at]))
    rescaled = ops.attention_rescale(mixed, S, valid=have.to(torch.int32))
    # where a frame was found this is the whole-recording track's own row
    assert bits(rescaled["maps"][have], A["maps"][at][have]) and bits(rescaled["range"][have], A["range"][at][have])
    return {"frame": frame, "count": torch.where(have, A["count"][at], torch.zeros_like(A["count"][at])), "mixed": mixed,
            "maps": rescaled["maps"], "range": rescaled["range"]}


def same(got, want, note):
    for k in ROW_KEYS:
        assert bits(got[k], want[k]), (note, k)


@pytest.mark.parametrize("shape, stride, per_call, max_age, Ra", [
    ("scalar", 2, 1, 1, 5), ("scalar", 2, 2, 2, 6), ("scalar", 1, 3, 4, 7), ("scalar", 3, 1, 5, 8), ("scalar", 2, 3, 3, 9),
    ("vector", 2, 1, 2, 5), ("vector", 2, 2, 2, 6), ("vector", 1, 3, 4, 7), ("vector", 3, 1, 5, 8), ("vector", 2, 3, 0, 9)])
def test_ring_rows_equal_the_offline_rule_on_the_windows_so_far(shape, stride, per_call, max_age, Ra):
    heads, Tp, T, h, w, local = SHAPES[shape]
    windows, chunk = 18, stride * per_call                      # frames that arrive between two calls
    assert Ra >= max(local[-1] - local[0] - stride + 1, chunk + max_age)          # the bound of stream.attention_ring_slots
    assert (windows - 1) * stride + local[-1] > 3 * Ra or stride == 1             # the ring turns
    col = columns(windows, shape, seed=3)
    frames = window_frames(shape, [wi * stride for wi in range(windows)])
    ring = ops.live_attention_ring(Ra, heads, h, w, DEV)
    seen = {"found": 0, "empty": 0, "shared": 0}
    for w0 in range(0, windows, per_call):
        w1 = min(w0 + per_call, windows)
        F = (w1 - 1) * stride + local[-1] + 1                   # frames in when the call's last window became ready
        f0 = max(0, F - chunk)
        add(ring, col[w0:w1], frames[w0:w1], live_from=max(0, f0 - max_age))
        got = ops.live_attention_rows(ring, f0, F - f0, S, max_age)
        want = offline(col[:w1], frames[:w1], f0, F - f0, T, max_age)
        same(got, want, (w0,))
        seen["found"] += int((got["frame"] >= 0).sum())
        seen["empty"] += int((got["frame"] < 0).sum())
        seen["shared"] += int((got["count"] > 1).sum())
    # frames gained pairs from several windows and calls; a row may hold its frame before the later pairs arrive (stride 3)
    assert seen["found"] > 0 and int(ring["count"].max()) > 1 and (seen["shared"] > 0 or stride == 3), seen
    assert ring["newest"] == int(frames.max()) and int(ring["frame"].max()) == ring["newest"]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_windows_of_one_call_that_share_a_frame_and_a_frame_that_grows_over_three_calls(shape):
    heads, Tp, T, h, w, local = SHAPES[shape]
    col = columns(4, shape, seed=5)
    last = local[-1]
    frames = window_frames(shape, [10, 10 + last, 10 + last, 10 + last - local[1]])      # frame 10 + last: windows 0, 1, 2 and more
    ring = ops.live_attention_ring(64, heads, h, w, DEV)
    add(ring, col[:2], frames[:2])                              # one call, two windows, both land on frame 10 + last
    n = 10 + last
    want = offline(col[:2], frames[:2], n, 1, T, 0)
    assert int(want["count"][0]) >= 2
    same(ops.live_attention_rows(ring, n, 1, S, 0), want, "one call")
    for upto in (3, 4):                                         # the same frame gains pairs over two more calls
        add(ring, col[upto - 1:upto], frames[upto - 1:upto])
        want = offline(col[:upto], frames[:upto], n, 1, T, 0)
        same(ops.live_attention_rows(ring, n, 1, S, 0), want, upto)
    assert int(want["count"][0]) >= 4
    same(ops.live_attention_rows(ring, 0, 40, S, 3), offline(col, frames, 0, 40, T, 3), "every frame")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ages_at_and_past_max_age_and_rows_before_frame_zero(shape):
    heads, Tp, T, h, w, local = SHAPES[shape]
    col = columns(1, shape, seed=7)
    frames = window_frames(shape, [2])
    newest = 2 + local[-1]
    ring = ops.live_attention_ring(9, heads, h, w, DEV)
    add(ring, col, frames)
    for max_age in (0, 1, 3):
        got = ops.live_attention_rows(ring, 0, newest + max_age + 3, S, max_age)      # from frame 0: n - max_age < 0 on the first rows
        same(got, offline(col, frames, 0, newest + max_age + 3, T, max_age), max_age)
        assert got["frame"][newest + max_age].item() == newest                         # exactly max_age old: held
        assert got["frame"][newest + max_age + 1].item() == -1                         # one older: empty
        empty = got["frame"] < 0
        assert bool(empty[:2].all()) and bool((got["count"][empty] == 0).all())
        assert bool((got["mixed"][empty] == 0).all()) and bool((got["maps"][empty] == 0).all())
        assert bool(torch.isnan(got["range"][empty]).all()) and not bool(torch.isnan(got["range"][~empty]).any())
        if max_age == 0:                                        # only the frames the window saw
            assert sorted(set(got["frame"][~empty].tolist())) == sorted(set(frames[0].tolist()))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_slot_recycled_by_a_frame_one_turn_later(shape):
    heads, Tp, T, h, w, local = SHAPES[shape]
    Ra = 7
    col = columns(2, shape, seed=9)
    first, second = window_frames(shape, [3]), window_frames(shape, [3 + Ra])
    ring = ops.live_attention_ring(Ra, heads, h, w, DEV)
    add(ring, col[:1], first, live_from=3)
    before = ops.live_attention_rows(ring, 3, 1, S, 0)
    assert before["frame"].item() == 3 and before["count"].item() == 1
    with pytest.raises(ValueError, match="would overwrite the slot of frame"):
        add(ring, col[1:], second, live_from=3)                 # frame 3 is still inside the live span
    add(ring, col[1:], second, live_from=3 + local[-1] + 1)
    assert ring["frame"][3 % Ra].item() == 3 + Ra and ring["count"][3 % Ra].item() == 1
    gone = ops.live_attention_rows(ring, 3, 1, S, 0)            # the slot holds another frame: empty for frame 3
    assert gone["frame"].item() == -1 and gone["count"].item() == 0 and bool(torch.isnan(gone["range"]).all())
    # the restarted slot holds the second window alone: 0 + its pairs, as attention_track sums them
    same(ops.live_attention_rows(ring, 3 + Ra, local[-1] + 1, S, 0), offline(col[1:], second, 3 + Ra, local[-1] + 1, T, 0), "restarted")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_negative_zero_restarts_to_plus_zero(shape):
    heads, Tp, T, h, w, local = SHAPES[shape]
    col = columns(2, shape, seed=11)
    col[:, 0, :, 0, :] = -0.0                                   # head 0, first row of cells, in every coarse map: m_p = -0 there
    frames = window_frames(shape, [0, 20])
    ring = ops.live_attention_ring(64, heads, h, w, DEV)
    ring["sum"].fill_(-1.0)                                     # a restart overwrites whatever the slot held
    add(ring, col, frames)
    slot = int(frames[1][0])                                    # a frame one pair landed on
    assert ring["count"][slot].item() == 1 or local[0] == local[1]
    cells = ring["sum"][slot, 0, 0].view(torch.int32)
    assert bool((cells == 0).all()), "0.f + (-0.f) is +0: the sign bit must be clear"
    got = ops.live_attention_rows(ring, 0, 30, S, 2)
    same(got, offline(col, frames, 0, 30, T, 2), "negative zero")
    assert bool((got["mixed"][slot, 0, 0].view(torch.int32) == 0).all())


def test_a_frame_with_one_pair_carries_audio_pixel_attn_of_that_pair():
    heads, Tp, T, h, w, hd = 3, 4, 8, 8, 8, 8
    g = torch.Generator().manual_seed(13)
    N = Tp * h * w + Tp
    qkv = torch.randn(1, N, 3 * heads * hd, generator=g).to(DEV)
    lse = torch.randn(1, heads, N, generator=g).to(DEV)
    apa = ops.audio_pixel_attn(qkv, lse, (Tp, h, w), heads, T, S)
    frames = 30 + 3 * np.arange(T, dtype=np.int64)[None]        # eight distinct frames: one pair each
    ring = ops.live_attention_ring(64, heads, h, w, DEV)
    add(ring, apa["column"], frames)
    got = ops.live_attention_rows(ring, 30, 3 * T, S, 2)
    for j in range(T):
        for n in range(30 + 3 * j, 30 + 3 * j + 3):             # the frame itself and the two that hold it
            assert got["frame"][n - 30].item() == 30 + 3 * j and got["count"][n - 30].item() == 1
            assert bits(got["maps"][n - 30], apa["maps"][0, :, j]) and bits(got["range"][n - 30], apa["range"][0, :, j])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_want_subsets_keep_their_bits_and_rows_only_read(shape):
    heads, Tp, T, h, w, local = SHAPES[shape]
    col = columns(3, shape, seed=15)
    frames = window_frames(shape, [0, 2, 9])
    ring = ops.live_attention_ring(32, heads, h, w, DEV)
    add(ring, col, frames)
    saved = {k: v.clone() for k, v in ring.items() if torch.is_tensor(v)}
    full = ops.live_attention_rows(ring, 0, 20, S, 2)
    assert sorted(full) == sorted(ROW_KEYS)
    for want in (("frame",), ("count", "frame"), ("mixed",), ("maps",), ("range",), ("maps", "range"), ("mixed", "range", "count")):
        part = ops.live_attention_rows(ring, 0, 20, S, 2, want=want)
        assert sorted(part) == sorted(want)
        for k in want:
            assert bits(part[k], full[k]), (want, k)
    for k in saved:
        assert torch.equal(ring[k], saved[k]), k


def test_refusals_leave_the_ring_untouched():
    heads, Tp, T, h, w, local = SHAPES["scalar"]
    Ra = 9
    col = columns(2, "scalar", seed=17)
    host = window_frames("scalar", [13, 14])                    # frames 13 .. 18
    dev = torch.from_numpy(host).to(DEV)
    ring = ops.live_attention_ring(Ra, heads, h, w, DEV)
    ops.live_attention_add(col, dev, host, ring, live_from=10)
    saved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ring.items()}
    assert saved["newest"] == 18
    low = np.array([[0, 1, 2, 4], [1, 2, 3, 5]], dtype=np.int64)
    down = np.array([[40, 30, 20, 12]], dtype=np.int64)
    bad = [
        (lambda: ops.live_attention_add(col.double(), dev, host, ring), ValueError, "fp32"),
        (lambda: ops.live_attention_add(col[:, :1], dev, host, ring), ValueError, "fp32"),
        (lambda: ops.live_attention_add(col[..., :4], dev, host, ring), ValueError, "fp32"),
        (lambda: ops.live_attention_add(col, dev.int(), host, ring), ValueError, "int64"),
        (lambda: ops.live_attention_add(col, dev[:1], host, ring), ValueError, "int64"),
        (lambda: ops.live_attention_add(col, dev, host[:1], ring), ValueError, "on the host"),
        (lambda: ops.live_attention_add(col, dev, dev, ring), ValueError, "host copy"),
        (lambda: ops.live_attention_add(col, dev - 20, host - 20, ring), ValueError, ">= 0"),
        (lambda: ops.live_attention_add(col.cpu(), dev, host, ring), lib.CstsError, "GPU"),
        (lambda: ops.live_attention_add(col, dev.cpu(), host, ring), lib.CstsError, "GPU"),
        (lambda: ops.live_attention_add(col, dev, host, dict(ring, sum=ring["sum"].cpu())), lib.CstsError, "GPU"),
        (lambda: ops.live_attention_add(col, dev, host, dict(ring, count=ring["count"].long())), ValueError, "int32"),
        (lambda: ops.live_attention_add(col, dev, host, dict(ring, frame=ring["frame"][:-1])), ValueError, "int64"),
        (lambda: ops.live_attention_add(col, dev, host, {"sum": ring["sum"]}), ValueError, "ops.live_attention_ring"),
        (lambda: ops.live_attention_add(col, dev, host, dict(ring, newest=8.0)), ValueError, "host int"),
        # frame 13 is still inside the live span: 13 + Ra would take its slot
        (lambda: ops.live_attention_add(col, dev + Ra, host + Ra, ring, live_from=13), ValueError, "would overwrite the slot of frame"),
        # frame 0 would land on the slot of frame 18, which is newer and in the ring already
        (lambda: ops.live_attention_add(col, torch.from_numpy(low).to(DEV), low, ring), ValueError, "slot of a newer frame"),
        # a window whose frames descend by a whole turn
        (lambda: ops.live_attention_add(col[:1], torch.from_numpy(down).to(DEV), down, ring, live_from=40), ValueError,
         "slot of a newer frame"),
        (lambda: ops.live_attention_rows(ring, 0, 0, S, 2), ValueError, "1..65535"),
        (lambda: ops.live_attention_rows(ring, -1, 4, S, 2), ValueError, "f0 >= 0"),
        (lambda: ops.live_attention_rows(ring, 0, 4, S, -1), ValueError, "max_age"),
        (lambda: ops.live_attention_rows(ring, 0, 4, 0, 2), ValueError, "crop_size"),
        (lambda: ops.live_attention_rows(ring, 0, 4, S, 2, want=("maps", "points")), ValueError, "want"),
        (lambda: ops.live_attention_rows(dict(ring, sum=ring["sum"].cpu()), 0, 4, S, 2), lib.CstsError, "GPU"),
        (lambda: ops.live_attention_ring(0, heads, h, w, DEV), ValueError, "slots"),
        (lambda: ops.live_attention_ring(8, heads, h, w, "cpu"), lib.CstsError, "MI355X"),
    ]
    for call, error, word in bad:
        with pytest.raises(error, match=word):
            call()
        for k in saved:
            assert (torch.equal(ring[k], saved[k]) if torch.is_tensor(saved[k]) else ring[k] == saved[k]), (word, k)
    ops.live_attention_add(col, dev + Ra, host + Ra, ring, live_from=19)    # the same windows once frames 13..18 are behind
    assert ring["newest"] == 27 and sorted(ring["frame"].tolist()) == [-1, -1, -1, 22, 23, 24, 25, 26, 27]
