"""csts_gaze_decode (csts_amd/csrc/decode.hip) against the float64 composition of the same logits on the CPU: frame_softmax at
temperature 2, the per-frame min-max rescale of tools/test_avgaze_net.py:68-70, the arg-max cell as a gaze point, the peak.
Bounds: preds and rescaled within the project's bar for this softmax (rel-L2 < 1e-5, tests/test_gpu_ops.py), peak within 1e-6
relative, points exactly equal on every frame."""
import os
import subprocess
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
SHAPES = {1: (1, 1), 8: (2, 4), 64: (4, 16)}            # frames -> (B, T)
GRIDS = (64, 56)                                         # 64^2 = 4096 (256 crop), 56^2 = 3136 (224 crop)


def rel_l2(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def reference(logits_cpu, temperature=2.0, unique=True):
    """The torch composition in float64 on the CPU.  logits (B, 1, T, H, W), any float type.  unique: assert that every frame
    has ONE maximum, so that its arg-max does not depend on a tie rule."""
    B, _, T, H, W = logits_cpu.shape
    z = logits_cpu.double().reshape(B * T, H * W)
    p = torch.softmax(z / temperature, dim=-1)
    mn, mx = p.min(dim=-1, keepdim=True).values, p.max(dim=-1, keepdim=True).values
    r = (p - mn) / (mx - mn + 1e-6)
    idx = z.argmax(dim=-1)
    if unique:
        assert bool(((z == z.max(dim=-1, keepdim=True).values).sum(dim=-1) == 1).all()), "the per-frame maximum must be unique"
    points = torch.stack([(idx % W).float() / W, torch.div(idx, W, rounding_mode="floor").float() / H], dim=-1)
    return {"preds": p.reshape(B, 1, T, H, W), "rescaled": r.reshape(B, 1, T, H, W), "points": points.reshape(B, T, 2),
            "peak": mx.reshape(B, T)}


def make_logits(n, g, dtype, seed):
    """Seeded logits (B, 1, T, g, g) with a unique per-frame maximum; 16-bit types get a distinct bump at a chosen cell."""
    B, T = SHAPES[n]
    x = torch.randn(B, 1, T, g, g, generator=torch.Generator().manual_seed(seed)) * 3
    if dtype != torch.float32:
        x = x.to(dtype)
        flat = x.view(B * T, g * g)
        for f in range(B * T):
            cell = (f * 977 + 13 + seed) % (g * g)
            flat[f, cell] = (flat[f].float().max() + 1.0).to(dtype)
    return x


def compare(out, ref, what):
    figures = {"preds": rel_l2(out["preds"], ref["preds"]), "rescaled": rel_l2(out["rescaled"], ref["rescaled"]),
               "peak": float(((out["peak"].cpu().double() - ref["peak"]).abs() / ref["peak"]).max()),
               "points_off": int((out["points"].cpu() != ref["points"]).any(dim=-1).sum())}
    print(f"gaze_decode {what}: {figures}")
    assert figures["preds"] < 1e-5, (what, figures)
    assert figures["rescaled"] < 1e-5, (what, figures)
    assert figures["peak"] < 1e-6, (what, figures)
    assert torch.equal(out["points"].cpu(), ref["points"]), (what, figures)          # every frame


def check_all_cases(dtypes):
    """Every (frames, grid, dtype) case.  Shared with tests/fp16_decode_worker.py, which runs it in the fp16 library."""
    for dtype in dtypes:
        for g in GRIDS:
            for n in SHAPES:
                x = make_logits(n, g, dtype, seed=100 + n + g)
                out = ops.gaze_decode(x.to(DEV), 2.0)
                assert set(out) == {"preds", "rescaled", "points", "peak"} and all(v.dtype == torch.float32 for v in out.values())
                assert out["preds"].shape == x.shape and out["points"].shape == (*SHAPES[n], 2) and out["peak"].shape == SHAPES[n]
                compare(out, reference(x), f"{n} frames of {g}x{g} {dtype}")
    return True


@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_fp32_logits(n, g):
    x = make_logits(n, g, torch.float32, seed=100 + n + g)
    compare(ops.gaze_decode(x.to(DEV), 2.0), reference(x), f"{n} frames of {g}x{g} fp32")


@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_16bit_logits_in_the_library_type(n, g):
    assert lib.half_dtype() == torch.bfloat16
    x = make_logits(n, g, torch.bfloat16, seed=100 + n + g)
    compare(ops.gaze_decode(x.to(DEV), 2.0), reference(x), f"{n} frames of {g}x{g} bf16")


def test_same_values_as_frame_softmax_and_the_metric_rescale():
    """preds is the heat map frame_softmax gives (same bar), at another temperature too."""
    x = make_logits(8, 64, torch.float32, seed=5).to(DEV)
    for temp in (2.0, 0.7):
        out = ops.gaze_decode(x, temp)
        assert rel_l2(out["preds"], ops.frame_softmax(x, temp)) < 1e-5
        compare(out, reference(x.cpu(), temp), f"temperature {temp}")


def test_frames_that_do_not_allow_vector_access():
    """H * W not a multiple of 4 (scalar path), a one-cell frame and the largest frame the header allows."""
    for (B, T, H, W) in ((2, 3, 7, 9), (1, 2, 1, 1), (1, 2, 64, 128), (1, 3, 30, 50)):
        x = torch.randn(B, 1, T, H, W, generator=torch.Generator().manual_seed(H * W)) * 3
        compare(ops.gaze_decode(x.to(DEV), 2.0), reference(x), f"{B * T} frames of {H}x{W}")
    x = torch.randn(1, 1, 2, 64, 128, generator=torch.Generator().manual_seed(3)) * 3
    buf = torch.empty(x.numel() + 1, device=DEV)
    buf[1:] = x.to(DEV).flatten()
    un = buf[1:].view(x.shape)                                # 4-byte aligned logits: the scalar path
    assert un.data_ptr() % 16 != 0
    compare(ops.gaze_decode(un, 2.0), reference(x), "unaligned logits")
    with pytest.raises(lib.CstsError, match="CSTS_GAZE_DECODE_MAX_HW"):
        ops.gaze_decode(torch.zeros(1, 1, 1, 64, 129, device=DEV))


def test_an_exact_tie_goes_to_the_lowest_flat_index():
    g = 64
    x = torch.randn(1, 1, 6, g, g, generator=torch.Generator().manual_seed(9))
    flat = x.view(6, g * g)
    top = float(flat.max()) + 2.0
    plants = [(4095, 1027, 2500), (5, 6), (4095,), (2048, 1024, 3072), (1023, 1020)]     # across waves / chunks, inside one lane
    for f, cells in enumerate(plants):
        flat[f, list(cells)] = top
    flat[5] = 0.25                                            # a constant frame: every cell ties
    want = [min(c) for c in plants] + [0]
    out = ops.gaze_decode(x.to(DEV), 2.0, want=("points", "peak"))
    pts = torch.tensor([[(i % g) / g, (i // g) / g] for i in want], dtype=torch.float32)
    assert torch.equal(out["points"].cpu().view(6, 2), pts)
    assert abs(float(out["peak"].view(-1)[5]) - 1.0 / (g * g)) < 1e-9
    x16 = x.to(lib.half_dtype())                              # the planted value is the same 16-bit number in every planted cell
    assert torch.equal(ops.gaze_decode(x16.to(DEV), 2.0, want=("points",))["points"].cpu().view(6, 2), pts)


def test_extreme_logits_give_finite_outputs():
    g = 64
    x = torch.full((1, 1, 4, g, g), -80.0)
    x.view(4, -1)[0, ::2] = 80.0                              # half the frame at +80, half at -80
    x.view(4, -1)[1, 77] = 80.0                               # one cell at +80
    x.view(4, -1)[2] = 80.0                                   # all at +80
    x.view(4, -1)[3, 4000] = -79.0                            # all but one at -80
    out = ops.gaze_decode(x.to(DEV), 2.0)
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
    assert torch.allclose(out["preds"].sum(dim=(-1, -2)).cpu(), torch.ones(1, 1, 4), atol=1e-5)
    assert float(out["rescaled"].min()) >= 0.0 and float(out["rescaled"].max()) <= 1.0
    ref = reference(x, unique=False)                          # frames 1 and 3 have a unique maximum
    assert torch.equal(out["points"].cpu()[0, 1], ref["points"][0, 1]) and torch.equal(out["points"].cpu()[0, 3], ref["points"][0, 3])
    assert torch.equal(out["points"].cpu()[0, 0], torch.zeros(2)) and torch.equal(out["points"].cpu()[0, 2], torch.zeros(2))


def test_null_outputs_are_skipped():
    x = make_logits(8, 56, torch.float32, seed=11).to(DEV)
    full = ops.gaze_decode(x, 2.0)
    only = ops.gaze_decode(x, 2.0, want=("points",))
    assert set(only) == {"points"} and torch.equal(only["points"], full["points"])
    two = ops.gaze_decode(x, 2.0, want=("rescaled", "peak"))
    assert set(two) == {"rescaled", "peak"} and torch.equal(two["rescaled"], full["rescaled"]) and torch.equal(two["peak"], full["peak"])
    with pytest.raises(ValueError):
        ops.gaze_decode(x, 2.0, want=("heat",))


def test_no_grad_only_and_capturable():
    x = make_logits(8, 64, torch.float32, seed=12).to(DEV)
    with pytest.raises(lib.CstsError, match="no backward"):
        ops.gaze_decode(x.clone().requires_grad_(True))
    with torch.no_grad():
        eager = ops.gaze_decode(x.clone().requires_grad_(True))
    static = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gaze_decode(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gaze_decode(static)                         # no host sync inside: the capture would fail on one
    y = make_logits(8, 64, torch.float32, seed=13)
    static.copy_(y.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    fresh = ops.gaze_decode(y.to(DEV))
    assert all(torch.equal(out[k], fresh[k]) for k in fresh)
    assert not torch.equal(eager["preds"], fresh["preds"])    # the replay saw the new logits


def test_fp16_library_runs_the_same_cases_in_a_fresh_process():
    env = dict(os.environ, CSTS_HALF="fp16")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fp16_decode_worker.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "fp16 decode cases passed" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
