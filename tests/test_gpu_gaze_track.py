"""csts_gaze_track (csts_amd/csrc/decode.hip, ops.gaze_track) against the float64 composition on the CPU: per output frame the
mean of the heat maps that target it, its min-max rescale, the arg-max cell as a gaze point, the peak and the count.

Bounds.  heatmaps: rel-L2 <= 1e-6 per frame -- at most 8 sequential fp32 additions plus one multiply, (K + 1) * 2^-24 = 5.4e-7
at K = 8 (the CPU emulation of that order on these inputs gives 6.0e-8).  rescaled: 1e-5 absolute.  peak: 1e-6 relative.
count: exact.  points: equal on every frame whose float64 top-two values differ by more than 1e-5 relative; closer frames may
be left out, at most 1 % of them (on these inputs the float64 reference leaves out none)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
F = 6
COUNTS = (0, 1, 2, 3, 8, 3)                      # frame 0 is empty; 8 is the deepest sum


def make_case(H, W, seed):
    """P = sum(COUNTS) + 1 maps softmax(randn / 2) in fp32 and their targets, interleaved so that no frame's rows are
    adjacent; one extra map targets a frame outside [0, F)."""
    g = torch.Generator().manual_seed(seed)
    targets = [f for f, n in enumerate(COUNTS) for _ in range(n)] + [F + 2]
    perm = torch.randperm(len(targets), generator=g)
    target_idx = torch.tensor(targets, dtype=torch.int64)[perm]
    preds = torch.softmax(torch.randn(len(targets), H * W, generator=g) / 2, dim=-1).reshape(-1, H, W)
    return preds, target_idx


def reference(preds, target_idx, H, W):
    """float64 on the CPU.  Returns the maps, points, peaks, counts and, per frame, whether its top two values are more than
    1e-5 relative apart."""
    p = preds.double().reshape(-1, H * W)
    heat = torch.zeros(F, H * W, dtype=torch.float64)
    count = torch.zeros(F, dtype=torch.int64)
    for row, t in enumerate(target_idx.tolist()):
        if 0 <= t < F:
            heat[t] += p[row]
            count[t] += 1
    heat = heat / count.clamp(min=1)[:, None]
    mn, mx = heat.min(dim=-1, keepdim=True).values, heat.max(dim=-1, keepdim=True).values
    resc = (heat - mn) / (mx - mn + 1e-6)
    top = heat.topk(2, dim=-1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-5 * top[:, 0]
    idx = heat.argmax(dim=-1)
    points = torch.stack([(idx % W).float() / W, torch.div(idx, W, rounding_mode="floor").float() / H], dim=-1)
    return {"heatmaps": heat.reshape(F, H, W), "rescaled": resc.reshape(F, H, W), "points": points, "peak": mx[:, 0],
            "count": count, "clear": clear}


def compare(out, ref, what):
    covered = ref["count"] > 0
    got_h, want_h = out["heatmaps"].cpu().double().reshape(F, -1), ref["heatmaps"].reshape(F, -1)
    rel = ((got_h - want_h).norm(dim=-1) / want_h.norm(dim=-1).clamp(min=1e-300))[covered]
    resc = float((out["rescaled"].cpu().double() - ref["rescaled"]).abs().max())
    peak = float(((out["peak"].cpu().double() - ref["peak"]).abs() / ref["peak"].clamp(min=1e-300))[covered].max())
    judged = covered & ref["clear"]
    left_out = int((covered & ~ref["clear"]).sum())
    off = int((out["points"].cpu()[judged] != ref["points"][judged]).any(dim=-1).sum())
    print(f"gaze_track {what}: heatmaps rel-L2 max {float(rel.max()):.3e}, rescaled abs {resc:.3e}, peak rel {peak:.3e}, "
          f"points off {off}, frames left out {left_out} of {int(covered.sum())}")
    assert float(rel.max()) <= 1e-6, what
    assert resc <= 1e-5, what
    assert peak <= 1e-6, what
    assert torch.equal(out["count"].cpu().long(), ref["count"]) and out["count"].dtype == torch.int32, what
    assert left_out <= 0.01 * int(covered.sum()), what
    assert off == 0, what
    # the empty frame: NaN points, zero maps, zero peak
    empty = ~covered
    assert int(empty.sum()) == 1
    assert bool(torch.isnan(out["points"].cpu()[empty]).all())
    assert float(out["heatmaps"].cpu()[empty].abs().max()) == 0.0 and float(out["rescaled"].cpu()[empty].abs().max()) == 0.0
    assert float(out["peak"].cpu()[empty].abs().max()) == 0.0
    assert bool(torch.isfinite(out["points"].cpu()[covered]).all())


@pytest.mark.parametrize("hw", [(64, 64), (56, 56), (7, 9)])
def test_against_the_float64_composition(hw):
    H, W = hw
    preds, target_idx = make_case(H, W, seed=H * W)
    ref = reference(preds, target_idx, H, W)
    out = ops.gaze_track(preds.to(DEV), target_idx.to(DEV), F)
    assert set(out) == {"heatmaps", "rescaled", "points", "peak", "count"}
    assert out["heatmaps"].shape == (F, H, W) and out["points"].shape == (F, 2) and out["peak"].shape == (F,)
    compare(out, ref, f"{H}x{W}")


def test_rows_are_added_in_ascending_order_and_the_result_is_deterministic():
    """The mean equals the fp32 emulation of the stated order bit for bit: ((0 + r0) + r1 + ...) * (1 / n)."""
    H = W = 64
    preds, target_idx = make_case(H, W, seed=7)
    out = ops.gaze_track(preds.to(DEV), target_idx.to(DEV), F, want=("heatmaps",))["heatmaps"].cpu()
    for f, n in enumerate(COUNTS):
        acc = torch.zeros(H, W)
        for row in (target_idx == f).nonzero().flatten().tolist():        # ascending row order
            acc = acc + preds[row]
        want = acc * (torch.tensor(1.0) / n) if n else acc
        assert torch.equal(out[f], want), f
    again = ops.gaze_track(preds.to(DEV), target_idx.to(DEV), F, want=("heatmaps",))["heatmaps"].cpu()
    assert torch.equal(out, again)


def test_unaligned_maps_take_the_scalar_path():
    H = W = 64
    preds, target_idx = make_case(H, W, seed=11)
    buf = torch.empty(preds.numel() + 1, device=DEV)
    buf[1:] = preds.to(DEV).flatten()
    un = buf[1:].view(preds.shape)
    assert un.data_ptr() % 16 != 0
    compare(ops.gaze_track(un, target_idx.to(DEV), F), reference(preds, target_idx, H, W), "unaligned 64x64")


def test_null_outputs_are_skipped_and_arguments_validated():
    H, W = 56, 56
    preds, target_idx = make_case(H, W, seed=5)
    p, t = preds.to(DEV), target_idx.to(DEV)
    full = ops.gaze_track(p, t, F)
    only = ops.gaze_track(p, t, F, want=("points",))
    assert set(only) == {"points"} and torch.equal(only["points"].nan_to_num(-1.0), full["points"].nan_to_num(-1.0))
    two = ops.gaze_track(p, t, F, want=("rescaled", "count"))
    assert set(two) == {"rescaled", "count"} and torch.equal(two["rescaled"], full["rescaled"]) and torch.equal(two["count"], full["count"])
    with pytest.raises(ValueError):
        ops.gaze_track(p, t, F, want=("heat",))
    with pytest.raises(ValueError):
        ops.gaze_track(p, t.int(), F)
    with pytest.raises(ValueError):
        ops.gaze_track(p, t[:-1], F)
    with pytest.raises(lib.CstsError, match="CSTS_GAZE_DECODE_MAX_HW"):
        ops.gaze_track(torch.zeros(2, 64, 129, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), 3)
    with pytest.raises(lib.CstsError):
        ops.gaze_track(preds, target_idx, F)


def test_capturable_no_host_read():
    H = W = 64
    preds, target_idx = make_case(H, W, seed=13)
    p, t = preds.to(DEV), target_idx.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gaze_track(p, t, F)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gaze_track(p, t, F)                              # a host read inside would fail the capture
    preds2, target2 = make_case(H, W, seed=14)
    p.copy_(preds2.to(DEV))
    t.copy_(target2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    fresh = ops.gaze_track(preds2.to(DEV), target2.to(DEV), F)
    assert all(torch.equal(out[k].nan_to_num(-1.0), fresh[k].nan_to_num(-1.0)) for k in fresh)
