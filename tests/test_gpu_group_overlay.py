"""The grouped overlay launch (csts_group_gaze_overlay / _yuv, csts_group_points_source; ops.group_gaze_overlay,
ops.group_points_source) against the single-tensor ops it restates: every job's bytes equal ops.gaze_overlay /
ops.gaze_overlay_yuv on that job alone, points_source and centers equal infer.points_to_source / marker_centers bit for bit, on
the GPU and on CPU tensors.  The first RGB job is also held to the float64 statement of tests/overlay_reference.py.

Bound of that last comparison, at alpha 0, 0.5 and 1: (1 - alpha) * frame, alpha * heat and their sum are exact in fp32 and in
float64 at these three alphas (halves of integers below 256), so a pixel can differ only where fp32 and float64 quantise the map
value to different q -- the close set of overlay_reference (|255 v - integer| <= 1e-3), where q is off by one and the JET colour
by one step of 4 a channel, i.e. the output by at most ceil(4 alpha).  Everywhere else the bytes are equal.  Close pixels are at
most 1 % of the blended ones (overlay_reference's cap)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import overlay_reference as R  # noqa: E402
from csts_amd import lib, marker_centers, ops, points_to_source  # noqa: E402

DEV = torch.device("cuda:0")
RADIUS = 3
# (K, H, W): vector path with a partial second band; byte path with a one-row band; baseline; one byte off alignment
RGB_JOBS = [(3, 40, 52), (1, 33, 30), (2, 64, 80), (1, 64, 80)]
# centres (X, Y): a disc straddling the band boundary (Y = 31), a negative X, a disc cut by the frame edge
RGB_CENTERS = [[(26, 31), (-1, -1), (50, 1)], [(15, 31)], [(0, 31), (-1, -1)], [(79, 63)]]
YUV_JOBS = [(2, 36, 44), (1, 34, 30), (1, 64, 80)]           # vector path; W % 4 == 2: the single-tensor op; baseline
YUV_CENTERS = [[(22, 31), (-1, -1)], [(29, 33)], [(40, 31)]]


def unaligned(frames):
    """The same frames one byte into a buffer: no dword alignment, so the byte path."""
    buf = torch.empty(frames.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = frames.flatten()
    un = buf[1:].view(frames.shape)
    assert un.data_ptr() % 4 != 0 and un.is_contiguous()
    return un


def _maps(n, m, g):
    p = torch.softmax(torch.randn(n, m * m, generator=g) / 2, dim=-1)
    mn, mx = p.min(dim=-1, keepdim=True).values, p.max(dim=-1, keepdim=True).values
    return ((p - mn) / (mx - mn + 1e-6)).reshape(n, m, m).contiguous()


def rgb_case(S, m):
    g = torch.Generator().manual_seed(1000 + S)
    host = [torch.randint(0, 256, (K, H, W, 3), generator=g, dtype=torch.uint8) for K, H, W in RGB_JOBS]
    frames = [f.to(DEV) for f in host]
    frames[3] = unaligned(frames[3])
    rows = [R.params_row(H, W, S, 1) for _, H, W in RGB_JOBS]
    P = sum(K for K, _, _ in RGB_JOBS)
    maps = _maps(P, m, g)
    centers = torch.tensor([c for job in RGB_CENTERS for c in job], dtype=torch.int32)
    return {"host": host, "frames": frames, "rows": rows, "maps": maps.to(DEV), "maps_host": maps, "centers": centers.to(DEV),
            "centers_host": centers, "S": S, "first": np.cumsum([0] + [K for K, _, _ in RGB_JOBS])}


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("S,m", [(32, 8), (256, 64)])
def test_rgb_jobs_equal_the_single_tensor_op_byte_for_byte(S, m, alpha):
    c = rgb_case(S, m)
    jobs = list(zip(c["frames"], c["rows"]))
    outs = ops.group_gaze_overlay(jobs, c["maps"], c["centers"], S, alpha=alpha, radius=RADIUS)
    assert len(outs) == 4 and len({o.untyped_storage().data_ptr() for o in outs}) == 1       # views of one allocation
    singles = []
    for j, (frames, row) in enumerate(jobs):
        sel = slice(int(c["first"][j]), int(c["first"][j + 1]))
        want = ops.gaze_overlay(frames, c["maps"][sel], row, S, centers=c["centers"][sel], alpha=alpha, radius=RADIUS)
        singles.append(want)
        assert outs[j].shape == frames.shape and outs[j].dtype == torch.uint8 and outs[j].data_ptr() % 16 == 0
        assert torch.equal(outs[j], want), j
        assert torch.equal(frames.cpu(), c["host"][j])                                # the input is not written
    assert torch.equal(outs[0][1], c["frames"][0][1]) and torch.equal(outs[2][1], c["frames"][2][1])     # negative X: untouched
    assert not torch.equal(outs[0][0], c["frames"][0][0])
    # in place: aligned clones, and job 3 inside its unaligned buffer
    work = [f.clone() for f in c["frames"][:3]] + [unaligned(c["frames"][3])]
    back = ops.group_gaze_overlay(list(zip(work, c["rows"])), c["maps"], c["centers"], S, alpha=alpha, radius=RADIUS, outs=work)
    assert all(b is w for b, w in zip(back, work))
    for j in range(4):
        assert torch.equal(work[j], singles[j]), j
    # given outputs and fresh ones mixed; an unaligned out leaves the vector path and gives the same bytes
    given = unaligned(torch.zeros_like(c["frames"][2]))
    mixed = ops.group_gaze_overlay(jobs, c["maps"], c["centers"], S, alpha=alpha, radius=RADIUS, outs=[None, None, given, None])
    assert mixed[2] is given and all(torch.equal(mixed[j], singles[j]) for j in range(4))
    # no markers at all
    none = ops.group_gaze_overlay(jobs[:2], c["maps"][:4], None, S, alpha=alpha)
    assert torch.equal(none[0], ops.gaze_overlay(jobs[0][0], c["maps"][:3], jobs[0][1], S, alpha=alpha))
    assert torch.equal(none[1], ops.gaze_overlay(jobs[1][0], c["maps"][3:4], jobs[1][1], S, alpha=alpha))


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("S,m", [(32, 8), (256, 64)])
def test_the_first_rgb_job_equals_the_float64_statement(S, m, alpha):
    c = rgb_case(S, m)
    outs = ops.group_gaze_overlay(list(zip(c["frames"], c["rows"])), c["maps"], c["centers"], S, alpha=alpha, radius=RADIUS)
    ref = R.reference(c["host"][0], c["maps_host"][:3], c["centers_host"][:3], c["rows"][0], S, alpha=alpha, radius=RADIUS)
    got = outs[0].cpu().numpy().astype(np.int64)
    diff = np.abs(got - ref["out"].astype(np.int64)).max(axis=-1)
    loose = ref["close"] & ~ref["marker"]
    blended = int(ref["heat"].sum())
    share = float(ref["close"].sum()) / max(blended, 1)
    print(f"group_gaze_overlay S {S} alpha {alpha}: {blended} blended pixels, close share {share:.4%}, off inside the close set: "
          f"{int(((diff > 0) & loose).sum())}, off outside it: {int(((diff > 0) & ~loose).sum())}")
    assert blended > 0 and int(ref["marker"].sum()) > 0 and share <= 0.01
    assert int(diff[~loose].max(initial=0)) == 0
    assert int(diff[loose].max(initial=0)) <= math.ceil(4 * alpha)


def yuv_case(pixel_format):
    S, m = 32, 8
    g = torch.Generator().manual_seed(77)
    host = [torch.randint(0, 256, (K, H * 3 // 2, W), generator=g, dtype=torch.uint8) for K, H, W in YUV_JOBS]
    rows = [R.params_row(H, W, S, 1) for _, H, W in YUV_JOBS]
    maps = _maps(sum(K for K, _, _ in YUV_JOBS), m, g).to(DEV)
    centers = torch.tensor([c for job in YUV_CENTERS for c in job], dtype=torch.int32, device=DEV)
    return {"host": host, "frames": [f.to(DEV) for f in host], "rows": rows, "maps": maps, "centers": centers, "S": S,
            "first": np.cumsum([0] + [K for K, _, _ in YUV_JOBS])}


@pytest.mark.parametrize("matrix,full_range", [("bt601", False), ("bt709", True)])
@pytest.mark.parametrize("pixel_format", ["nv12", "i420"])
def test_yuv_jobs_equal_the_single_tensor_op_and_only_the_odd_width_reaches_it(pixel_format, matrix, full_range, monkeypatch):
    c = yuv_case(pixel_format)
    fmt = {"pixel_format": pixel_format, "matrix": matrix, "full_range": full_range}
    jobs = list(zip(c["frames"], c["rows"]))
    singles = []
    for j, (frames, row) in enumerate(jobs):
        sel = slice(int(c["first"][j]), int(c["first"][j + 1]))
        singles.append(ops.gaze_overlay_yuv(frames, c["maps"][sel], row, c["S"], centers=c["centers"][sel], alpha=0.5, radius=RADIUS,
                                            **fmt))
        assert not torch.equal(singles[j], frames)
    seen = []
    single = ops.gaze_overlay_yuv

    def counted(frames, *args, **kwargs):
        seen.append(tuple(frames.shape))
        return single(frames, *args, **kwargs)

    monkeypatch.setattr(ops, "gaze_overlay_yuv", counted)
    outs = ops.group_gaze_overlay(jobs, c["maps"], c["centers"], c["S"], alpha=0.5, radius=RADIUS, **fmt)
    assert seen == [(1, 51, 30)]                                  # the W % 4 == 2 job, and no other
    assert len({o.untyped_storage().data_ptr() for o in outs}) == 1
    for j in range(3):
        assert outs[j].data_ptr() % 16 == 0 and torch.equal(outs[j], singles[j]), j
        assert torch.equal(c["frames"][j].cpu(), c["host"][j])
    assert torch.equal(outs[0][1], c["frames"][0][1])             # negative X: the frame comes back byte for byte
    work = [f.clone() for f in c["frames"]]
    back = ops.group_gaze_overlay(list(zip(work, c["rows"])), c["maps"], c["centers"], c["S"], alpha=0.5, radius=RADIUS, outs=work,
                                  **fmt)
    assert all(b is w for b, w in zip(back, work)) and len(seen) == 2
    for j in range(3):
        assert torch.equal(work[j], singles[j]), j
    # a misaligned view of a vector-width job also leaves the launch and keeps its bytes
    off = unaligned(c["frames"][2])
    again = ops.group_gaze_overlay([jobs[0], (off, c["rows"][2])], torch.cat([c["maps"][:2], c["maps"][3:4]]),
                                   torch.cat([c["centers"][:2], c["centers"][3:4]]), c["S"], alpha=0.5, radius=RADIUS, **fmt)
    assert seen[-1] == (1, 96, 80) and len(seen) == 3
    assert torch.equal(again[0], singles[0]) and torch.equal(again[1], singles[2])


# ---- group_points_source ------------------------------------------------------------------------------------------------------
POINT_JOBS = [((341, 256, 42, 0, 0), 48, 36), ((256, 455, 0, 99, 0), 1080, 1920), ((256, 256, 0, 0, 0), 256, 256)]


def _points():
    """Per job: random fp32 points in [0, 1), then the specials on x against the specials rotated by one on y."""
    g = torch.Generator().manual_seed(4096)
    special = torch.tensor([float("nan"), 0.0, float.fromhex("0x1p-149"), float(np.nextafter(np.float32(1), np.float32(0)))] +
                           [(k + 0.5) / 64 for k in range(64)], dtype=torch.float32)
    parts, counts = [], []
    for n in (1365, 1365, 1366):
        rand = torch.rand(n, 2, generator=g, dtype=torch.float32)
        parts += [rand, torch.stack([special, special.roll(1)], dim=-1)]
        counts.append(n + special.numel())
    return torch.cat(parts), counts


@pytest.fixture(scope="module")
def points_case():
    points, counts = _points()
    assert points.shape[0] == 4096 + 3 * 68 and bool((points[~points.isnan()] < 1).all())
    jobs = [(K, list(row), H, W) for K, (row, H, W) in zip(counts, POINT_JOBS)]
    got = ops.group_points_source(points.to(DEV), jobs, 256)
    return points, jobs, got


@pytest.mark.parametrize("where", ["gpu", "cpu"])
def test_points_source_and_centers_equal_the_torch_composition_bit_for_bit(points_case, where):
    points, jobs, got = points_case
    assert got["points_source"].dtype == torch.float64 and got["centers"].dtype == torch.int32
    assert tuple(got["points_source"].shape) == tuple(got["centers"].shape) == (points.shape[0], 2)
    at = 0
    for K, row, H, W in jobs:
        p = points[at:at + K].to(DEV) if where == "gpu" else points[at:at + K]
        src = points_to_source(p, row, 256)
        cen = marker_centers(src, H, W)
        mine = got["points_source"][at:at + K].to(src.device)
        assert torch.equal(mine.view(torch.int64), src.contiguous().view(torch.int64)), (where, row)
        assert torch.equal(got["centers"][at:at + K].to(cen.device), cen), (where, row)
        nan = p.isnan().any(dim=-1).to(cen.device)
        assert int(nan.sum()) == 2 and bool((cen[nan] == -1).all()) and bool((cen[~nan] >= 0).all())
        at += K


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = rgb_case(32, 8)
    jobs = list(zip(c["frames"], c["rows"]))
    args = (c["maps"], c["centers"], 32)
    with pytest.raises(ValueError, match=r"rescaled must be fp32 \(7, mh, mw\)"):
        ops.group_gaze_overlay(jobs, c["maps"][:6], c["centers"], 32)
    with pytest.raises(ValueError, match=r"centers must be int32 \(7, 2\)"):
        ops.group_gaze_overlay(jobs, c["maps"], c["centers"][:6], 32)
    with pytest.raises(ValueError, match=r"^job 1: .*flip != 0"):
        ops.group_gaze_overlay([jobs[0], (c["frames"][1], c["rows"][1][:4] + [1]), jobs[2], jobs[3]], *args)
    with pytest.raises(ValueError, match=r"^job 2: .*do not hold a 32 x 32 crop"):
        ops.group_gaze_overlay([jobs[0], jobs[1], (c["frames"][2], [31, 40, 0, 0, 0]), jobs[3]], *args)
    wide = torch.zeros(1, 2, 8196, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match=r"^job 0: .*8192"):
        ops.group_gaze_overlay([(wide, [32, 131136, 0, 0, 0])], c["maps"][:1], c["centers"][:1], 32)
    with pytest.raises(ValueError, match=r"^job 3: out overlaps the frames of job 2"):          # job 3 writes what job 2 reads
        ops.group_gaze_overlay(jobs[:2] + [jobs[2], (c["frames"][2][:1], c["rows"][2])], *args,
                               outs=[None, None, None, c["frames"][2][1:]])
    shared = torch.empty_like(c["frames"][2])
    with pytest.raises(ValueError, match=r"out overlaps the out of job"):
        ops.group_gaze_overlay([jobs[2], jobs[2]], c["maps"][:4], c["centers"][:4], 32, outs=[shared, shared])
    with pytest.raises(ValueError, match=r"^job 0: out must be the frames themselves"):
        ops.group_gaze_overlay([(c["frames"][0][:2], c["rows"][0])], c["maps"][:2], c["centers"][:2], 32, outs=[c["frames"][0][1:]])
    with pytest.raises(lib.CstsError, match=r"^job 1: .*CPU tensor"):
        ops.group_gaze_overlay([jobs[0], (c["frames"][1].cpu(), c["rows"][1])] + jobs[2:], *args)
    with pytest.raises(lib.CstsError, match="CPU tensor"):
        ops.group_gaze_overlay(jobs, c["maps"].cpu(), c["centers"], 32)
    with pytest.raises(ValueError, match=r"^job 0: .*contiguous"):
        ops.group_gaze_overlay([(c["frames"][0][:, ::2], c["rows"][0])], c["maps"][:3], c["centers"][:3], 32)
    with pytest.raises(ValueError, match="one entry per job"):
        ops.group_gaze_overlay(jobs, *args, outs=[None])
    with pytest.raises(ValueError, match="alpha must lie in"):
        ops.group_gaze_overlay(jobs, *args, alpha=1.5)
    with pytest.raises(ValueError, match="1..65535 jobs"):
        ops.group_gaze_overlay([], c["maps"][:0], c["centers"][:0], 32)
    assert all(torch.equal(f.cpu(), h) for f, h in zip(c["frames"], c["host"]))       # a refusal writes nothing
    points = torch.rand(5, 2, device=DEV)
    with pytest.raises(ValueError, match=r"points must be fp32 \(6, 2\)"):
        ops.group_points_source(points, [(6, [32, 32, 0, 0, 0], 40, 52)], 32)
    with pytest.raises(ValueError, match=r"^job 1: .*out of range"):
        ops.group_points_source(points, [(2, [32, 32, 0, 0, 0], 40, 52), (3, [0, 32, 0, 0, 0], 40, 52)], 32)
    with pytest.raises(ValueError, match=r"^job 0: "):
        ops.group_points_source(points, [(0, [32, 32, 0, 0, 0], 40, 52), (5, [32, 32, 0, 0, 0], 40, 52)], 32)
    with pytest.raises(lib.CstsError, match="CPU tensor"):
        ops.group_points_source(points.cpu(), [(5, [32, 32, 0, 0, 0], 40, 52)], 32)
