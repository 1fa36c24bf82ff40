"""csts_gaze_track_fill (csts_amd/csrc/decode.hip, ops.gaze_track_fill) against the float64 composition on the CPU.

Inputs: F = 20 frames; four maps softmax(randn(4, H * W, seed H * W) / 2) placed at frames (3, 6, 7, 16) by ops.gaze_track, one
row per frame, so the mean is the map itself; its heatmaps and count go into gaze_track_fill.  Both modes, max_gap 4 and 9.

Bounds.  Predicted frames: every output bit-equal to gaze_track's.  neighbours: equal to infer.fill_plan.  Unfilled frames: zero
maps, NaN points, zero peak.  hold: all four outputs of a filled frame bit-equal to frame a's.  linear heatmaps: rel-L2 <= 1e-6
per filled frame -- all terms are positive and each of two divisions, two multiplies and one add is correctly rounded, so
element-wise 3 * 2^-24 = 1.8e-7 (the fp32 emulation on the CPU gives 5e-8 on these inputs).  linear rescaled 1e-5 absolute, peak
1e-6 relative (the bounds of tests/test_gpu_gaze_track.py), map sum 1 within 1e-5.  linear points: equal on every frame whose
float64 top-two values differ by more than 1e-5 relative; closer frames may be left out, at most 1 % of the covered frames (the
float64 reference leaves out none on these inputs)."""
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

from csts_amd import fill_plan, lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
F = 20
PREDICTED = (3, 6, 7, 16)
SHAPES = [(64, 64), (56, 56), (7, 9), (64, 128)]
_CASES = {}


def sparse_track(H, W, predicted=PREDICTED, seed=None):
    """The maps on the CPU and gaze_track's outputs for them on the device (computed once per shape and left unchanged)."""
    key = (H, W, predicted, seed)
    if key not in _CASES:
        g = torch.Generator().manual_seed(H * W if seed is None else seed)
        maps = torch.softmax(torch.randn(len(predicted), H * W, generator=g) / 2, dim=-1).reshape(-1, H, W)
        target = torch.tensor(predicted, dtype=torch.int64)
        _CASES[key] = (maps, ops.gaze_track(maps.to(DEV), target.to(DEV), F))
    return _CASES[key]


def reference(maps, H, W, mode, max_gap, predicted=PREDICTED):
    """float64 on the CPU: the filled maps, their rescale, points and peak, and per frame whether its top two values are more
    than 1e-5 relative apart."""
    count = np.zeros(F, dtype=np.int32)
    count[list(predicted)] = 1
    nb = fill_plan(count, max_gap)
    src = {f: maps[i].double().reshape(-1) for i, f in enumerate(predicted)}
    heat = torch.zeros(F, H * W, dtype=torch.float64)
    for n, (a, b) in enumerate(nb.tolist()):
        if a < 0:
            continue
        if a == b or mode == "hold":
            heat[n] = src[a]
        else:
            heat[n] = ((b - n) * src[a] + (n - a) * src[b]) / (b - a)
    mn, mx = heat.min(dim=-1, keepdim=True).values, heat.max(dim=-1, keepdim=True).values
    resc = (heat - mn) / (mx - mn + 1e-6)
    top = heat.topk(2, dim=-1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-5 * top[:, 0]
    idx = heat.argmax(dim=-1)
    points = torch.stack([(idx % W).float() / W, torch.div(idx, W, rounding_mode="floor").float() / H], dim=-1)
    return {"heatmaps": heat, "rescaled": resc, "points": points, "peak": mx[:, 0], "clear": clear, "neighbours": nb,
            "count": count}


def check(out, sparse, ref, mode, what):
    nb, count = ref["neighbours"], ref["count"]
    got = {k: v.cpu() for k, v in out.items()}
    base = {k: v.cpu() for k, v in sparse.items()}
    assert got["neighbours"].dtype == torch.int32 and np.array_equal(got["neighbours"].numpy().astype(np.int64), nb), what
    predicted = torch.from_numpy(count > 0)
    covered = torch.from_numpy(nb[:, 0] >= 0)
    filled = covered & ~predicted
    # predicted frames: the bits of gaze_track
    for k in ("heatmaps", "rescaled", "points", "peak"):
        assert torch.equal(got[k][predicted], base[k][predicted]), (what, k)
    # unfilled frames
    empty = ~covered
    assert int(empty.sum()) >= 6
    assert bool(torch.isnan(got["points"][empty]).all()) and bool(torch.isfinite(got["points"][covered]).all()), what
    assert float(got["heatmaps"][empty].abs().max()) == 0.0 and float(got["rescaled"][empty].abs().max()) == 0.0, what
    assert float(got["peak"][empty].abs().max()) == 0.0, what
    if not bool(filled.any()):
        return
    frames = filled.nonzero().flatten().tolist()
    if mode == "hold":
        for n in frames:
            a = int(nb[n, 0])
            for k in ("heatmaps", "rescaled", "points", "peak"):
                assert torch.equal(got[k][n], base[k][a]), (what, k, n)
        return
    got_h, want_h = got["heatmaps"].double().reshape(F, -1), ref["heatmaps"]
    rel = ((got_h - want_h).norm(dim=-1) / want_h.norm(dim=-1).clamp(min=1e-300))[filled]
    resc = float((got["rescaled"].double().reshape(F, -1) - ref["rescaled"])[covered].abs().max())
    peak = float(((got["peak"].double() - ref["peak"]).abs() / ref["peak"].clamp(min=1e-300))[covered].max())
    total = float((got_h.sum(dim=-1) - 1.0)[covered].abs().max())
    judged = covered & ref["clear"]
    left_out = int((covered & ~ref["clear"]).sum())
    off = int((got["points"][judged] != ref["points"][judged]).any(dim=-1).sum())
    print(f"gaze_track_fill {what}: heatmaps rel-L2 max {float(rel.max()):.3e}, rescaled abs {resc:.3e}, peak rel {peak:.3e}, "
          f"|sum - 1| {total:.3e}, points off {off}, frames left out {left_out} of {int(covered.sum())}")
    assert float(rel.max()) <= 1e-6, what
    assert resc <= 1e-5, what
    assert peak <= 1e-6, what
    assert total <= 1e-5, what
    assert left_out <= 0.01 * int(covered.sum()), what
    assert off == 0, what


@pytest.mark.parametrize("max_gap", [4, 9])
@pytest.mark.parametrize("mode", ["hold", "linear"])
@pytest.mark.parametrize("hw", SHAPES)
def test_against_the_float64_composition(hw, mode, max_gap):
    H, W = hw
    maps, sparse = sparse_track(H, W)
    out = ops.gaze_track_fill(sparse["heatmaps"], sparse["count"], mode=mode, max_gap=max_gap)
    assert set(out) == {"heatmaps", "rescaled", "points", "peak", "neighbours"}
    assert out["heatmaps"].shape == (F, H, W) and out["rescaled"].shape == (F, H, W)
    assert out["points"].shape == (F, 2) and out["peak"].shape == (F,) and out["neighbours"].shape == (F, 2)
    assert out["heatmaps"].data_ptr() != sparse["heatmaps"].data_ptr()
    check(out, sparse, reference(maps, H, W, mode, max_gap), mode, f"{H}x{W} {mode} gap {max_gap}")


def test_linear_is_the_stated_fp32_arithmetic():
    """wa * H_a + wb * H_b with wa = fl(fl(b - n) / fl(b - a)), wb likewise: the CPU's fp32 gives the same bits."""
    H = W = 64
    maps, sparse = sparse_track(H, W)
    out = ops.gaze_track_fill(sparse["heatmaps"], sparse["count"], mode="linear", max_gap=9, want=("heatmaps",))["heatmaps"].cpu()
    src = dict(zip(PREDICTED, maps))
    for n, (a, b) in enumerate(fill_plan((sparse["count"] > 0).cpu().numpy(), 9).tolist()):
        if a < 0 or a == b:
            continue
        span = torch.tensor(float(b - a))
        wa, wb = torch.tensor(float(b - n)) / span, torch.tensor(float(n - a)) / span
        assert torch.equal(out[n], wa * src[a] + wb * src[b]), n


@pytest.mark.parametrize("mode", ["hold", "linear"])
def test_unaligned_maps_take_the_scalar_path(mode):
    H = W = 64
    maps, sparse = sparse_track(H, W)
    buf = torch.empty(F * H * W + 1, device=DEV)
    buf[1:] = sparse["heatmaps"].flatten()
    un = buf[1:].view(F, H, W)
    assert un.data_ptr() % 16 != 0
    out = ops.gaze_track_fill(un, sparse["count"], mode=mode, max_gap=9)
    check(out, sparse, reference(maps, H, W, mode, 9), mode, f"unaligned 64x64 {mode}")
    aligned = ops.gaze_track_fill(sparse["heatmaps"], sparse["count"], mode=mode, max_gap=9)
    for k in aligned:
        assert torch.equal(out[k].nan_to_num(-1.0), aligned[k].nan_to_num(-1.0)), k


def test_want_subsets_skip_outputs_and_arguments_are_validated():
    H, W = 56, 56
    _, sparse = sparse_track(H, W)
    h, c = sparse["heatmaps"], sparse["count"]
    full = ops.gaze_track_fill(h, c, max_gap=9)
    only = ops.gaze_track_fill(h, c, max_gap=9, want=("points",))
    assert set(only) == {"points"} and torch.equal(only["points"].nan_to_num(-1.0), full["points"].nan_to_num(-1.0))
    two = ops.gaze_track_fill(h, c, max_gap=9, want=("rescaled", "neighbours"))
    assert set(two) == {"rescaled", "neighbours"} and torch.equal(two["rescaled"], full["rescaled"])
    assert torch.equal(two["neighbours"], full["neighbours"])
    with pytest.raises(ValueError):
        ops.gaze_track_fill(h, c, want=("count",))
    with pytest.raises(ValueError):
        ops.gaze_track_fill(h, c, want=())
    with pytest.raises(ValueError):
        ops.gaze_track_fill(h, c, mode="nearest")
    with pytest.raises(ValueError):
        ops.gaze_track_fill(h, c.long())
    with pytest.raises(ValueError):
        ops.gaze_track_fill(h, c[:-1])
    with pytest.raises(ValueError):
        ops.gaze_track_fill(h.double(), c)
    with pytest.raises(lib.CstsError, match="CSTS_GAZE_FILL_MAX_GAP"):
        ops.gaze_track_fill(h, c, max_gap=0)
    with pytest.raises(lib.CstsError, match="CSTS_GAZE_FILL_MAX_GAP"):
        ops.gaze_track_fill(h, c, max_gap=1025)
    with pytest.raises(lib.CstsError, match="CSTS_GAZE_DECODE_MAX_HW"):
        ops.gaze_track_fill(torch.zeros(2, 64, 129, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(lib.CstsError):
        ops.gaze_track_fill(h.cpu(), c.cpu())


def test_the_largest_gap_and_two_calls_give_equal_bits():
    """max_gap at the cap fills every hole between the first and the last prediction; a second call gives the same bits."""
    H = W = 64
    maps, sparse = sparse_track(H, W)
    a = ops.gaze_track_fill(sparse["heatmaps"], sparse["count"], mode="linear", max_gap=1024)
    b = ops.gaze_track_fill(sparse["heatmaps"], sparse["count"], mode="linear", max_gap=1024)
    for k in a:
        assert torch.equal(a[k].nan_to_num(-1.0), b[k].nan_to_num(-1.0)), k
    check(a, sparse, reference(maps, H, W, "linear", 1024), "linear", "64x64 linear gap 1024")
    covered = (a["neighbours"][:, 0] >= 0).cpu()
    assert covered.nonzero().flatten().tolist() == list(range(3, 17))


def test_capturable_no_host_read():
    H = W = 64
    _, first = sparse_track(H, W)
    h, c = first["heatmaps"].clone(), first["count"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gaze_track_fill(h, c, mode="linear", max_gap=9)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gaze_track_fill(h, c, mode="linear", max_gap=9)      # a host read inside would fail the capture
    other = (0, 5, 13, 19)
    maps2, second = sparse_track(H, W, predicted=other, seed=14)
    assert not torch.equal(second["count"], first["count"])
    h.copy_(second["heatmaps"])
    c.copy_(second["count"])
    graph.replay()
    torch.cuda.synchronize()
    fresh = ops.gaze_track_fill(second["heatmaps"], second["count"], mode="linear", max_gap=9)
    for k in fresh:
        assert torch.equal(out[k].nan_to_num(-1.0), fresh[k].nan_to_num(-1.0)), k
    want = fill_plan(second["count"].cpu().numpy(), 9)
    assert np.array_equal(out["neighbours"].cpu().numpy().astype(np.int64), want)
    assert (want[1:5] == (0, 5)).all() and (want[6:13] == (5, 13)).all() and (want[14:19] == (13, 19)).all()
