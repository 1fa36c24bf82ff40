"""csts_audio_pixel_attn at kernel level (ops.audio_pixel_attn) against tests/attention_reference.py.  The test builds random
packed qkv and computes the rows' log-sum-exp itself in float64 torch, with the spatial mask, in the log2 domain: it depends on
no other kernel for its inputs.

Tolerance of `column`: not a fixed number.  The parent's ops.attention_probs is measured against the same float64 softmax on the
same inputs (maximum relative error over the column's entries), and the new kernel is allowed twice that: it adds the same
head_dim products in another order and takes one exp2.  Both figures are printed."""
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

import attention_reference as A  # noqa: E402
import overlay_reference as OR  # noqa: E402
from csts_amd import lib as L  # noqa: E402
from csts_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
RUNS = [(name, False) for name in sorted(A.CASES)] + [("shipped", True)]
IDS = [n + ("_half" if h else "") for n, h in RUNS]
_DONE = {}


def _run(name, half):
    """One launch of the kernel and one of the parent's attention_probs per case, shared by the tests."""
    key = (name, half)
    if key not in _DONE:
        B, Hh, hd, Tp, h, w, T, S, _ = A.CASES[name]
        case = A.kernel_case(name, L.half_dtype() if half else None)
        qkv, lse = case["qkv"].to(DEV), case["lse"].to(DEV)
        out = ops.audio_pixel_attn(qkv, lse, (Tp, h, w), Hh, T, S)
        N = Tp * h * w + Tp
        probs = ops.attention_probs(qkv, B, N, Hh * hd, Hh, lse, L.MASK_SPATIAL, Tp, h * w)
        torch.cuda.synchronize()
        cut = A.cut_column(probs.cpu().numpy(), Tp, h * w).reshape(B, Hh, Tp, h, w)
        _DONE[key] = ({k: v.cpu().numpy() for k, v in out.items()}, cut, case["column"], out["maps"])
    return _DONE[key]


def _rel(got, want):
    return float((np.abs(got.astype(np.float64) - want) / np.abs(want)).max())


@pytest.mark.parametrize("name,half", RUNS, ids=IDS)
def test_column_against_float64_and_the_slices_of_attention_probs(name, half):
    out, cut, want, _ = _run(name, half)
    B, Hh, hd, Tp, h, w, T, S, _ = A.CASES[name]
    assert out["column"].shape == (B, Hh, Tp, h, w) and out["column"].dtype == np.float32
    e_probs, e_new = _rel(cut, want), _rel(out["column"], want)
    e_slice = float((np.abs(out["column"].astype(np.float64) - cut.astype(np.float64)) / np.abs(want)).max())
    print(f"audio_pixel_attn {name}{' half' if half else ''}: max relative error against float64: attention_probs {e_probs:.3e}, "
          f"new kernel {e_new:.3e} (allowed {2 * e_probs:.3e}); new kernel against the slices of attention_probs {e_slice:.3e}")
    assert e_probs > 0 and np.isfinite(out["column"]).all()
    assert e_new <= 2 * e_probs
    assert e_slice <= 2 * e_probs


@pytest.mark.parametrize("name,half", RUNS, ids=IDS)
def test_column_mean_is_the_ascending_fp32_mean(name, half):
    out = _run(name, half)[0]
    col = out["column"]
    s = np.zeros_like(col[:, 0])
    for k in range(col.shape[1]):
        s = s + col[:, k]
    assert s.dtype == np.float32
    assert np.array_equal(out["column_mean"], s / np.float32(col.shape[1]))


@pytest.mark.parametrize("name,half", RUNS, ids=IDS)
def test_range_and_maps_against_the_float64_restatement(name, half):
    """From the kernel's own column on: the float64 restatement of the mix in time, the lattice extrema and the rescale.  range
    within 1e-6 max|column| (about 4 fp32 ulps of a convex combination); maps through the picture they are for: drawn by
    gaze_overlay on an S x S identity crop they match the restatement under overlay_reference.compare's bound."""
    out, _, _, maps_dev = _run(name, half)
    B, Hh, hd, Tp, h, w, T, S, seed = A.CASES[name]
    r = A.restate(out["column"], T, S)
    assert out["maps"].shape == (B, Hh + 1, T, h, w) and out["range"].shape == (B, Hh + 1, T, 2)
    full = A.lattice_range(r["mixed"], S)
    assert np.array_equal(np.stack(full, axis=-1), r["range"])                      # end pixels == whole lattice, float64
    err = float(np.abs(out["range"].astype(np.float64) - r["range"]).max())
    bound = 1e-6 * float(np.abs(out["column"]).max())
    print(f"audio_pixel_attn {name}: range off by {err:.3e}, allowed {bound:.3e}")
    assert err <= bound
    n = B * (Hh + 1) * T
    frames = torch.randint(0, 256, (n, S, S, 3), generator=torch.Generator().manual_seed(seed + 50), dtype=torch.uint8)
    row = [S, S, 0, 0, 0]
    got = ops.gaze_overlay(frames.to(DEV), maps_dev.reshape(n, h, w), row, S)
    ref = OR.reference(frames, r["maps"].reshape(n, h, w), None, row, S)
    OR.compare(got, ref, f"fusion maps {name}{' half' if half else ''}")


def test_time_identity_passes_the_column_through():
    out = _run("time_identity", False)[0]
    col = np.concatenate([out["column"], out["column_mean"][:, None]], axis=1)
    lo, hi = out["range"][..., 0, None, None], out["range"][..., 1, None, None]
    assert np.array_equal(out["maps"], (col - lo) / (hi - lo + np.float32(1e-6)))


def test_bad_arguments_raise():
    B, Hh, hd, Tp, h, w, T, S, _ = A.CASES["grid_5x5"]
    case = A.kernel_case("grid_5x5")
    qkv, lse = case["qkv"].to(DEV), case["lse"].to(DEV)
    with pytest.raises(ValueError):
        ops.audio_pixel_attn(qkv, lse, (Tp, h, w + 1), Hh, T, S)          # N does not fit the grid
    with pytest.raises(ValueError):
        ops.audio_pixel_attn(qkv[:, :-1], lse[:, :, :-1], (Tp, h, w), Hh, T, S)
    with pytest.raises(ValueError):
        ops.audio_pixel_attn(qkv, lse, (Tp, h, w), Hh, 0, S)              # T < 1
    with pytest.raises(ValueError):
        ops.audio_pixel_attn(qkv, lse.double(), (Tp, h, w), Hh, T, S)
    with pytest.raises(L.CstsError):
        ops.audio_pixel_attn(qkv.clone().requires_grad_(True), lse, (Tp, h, w), Hh, T, S)
    with torch.no_grad():                                                 # the same tensor is fine where no tape runs
        ops.audio_pixel_attn(qkv.clone().requires_grad_(True), lse, (Tp, h, w), Hh, T, S)
    with pytest.raises(L.CstsError):
        ops.audio_pixel_attn(qkv.cpu(), lse.cpu(), (Tp, h, w), Hh, T, S)
    # a size the kernel does not assume is refused by its own guard, not run
    with pytest.raises(L.CstsError):
        ops.audio_pixel_attn(torch.zeros(1, 2 * 129 + 2, 3 * 8, device=DEV), torch.zeros(1, 1, 2 * 129 + 2, device=DEV), (2, 129, 1), 1, 2, 16)
