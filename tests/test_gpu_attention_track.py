"""csts_attention_track / csts_attention_rescale at kernel level against tests/attention_track_reference.py.

`column` is what ops.audio_pixel_attn computes from the random qkv / lse of the case (softmax-like, positive fp32), so the same
launch also gives the one-clip maps a frame with one pair must equal bit for bit.  The C entry is called on buffers with
NaN-filled guard regions and on pair lists built on the host; ops.attention_track (lists built on the device) must give the same
bits.

Bounds: mixed, count and maps bit for bit (every step of the rule is one IEEE fp32 operation); range within 1e-6 max|mixed| of the
float64 extrema of the kernel's own mixed, the bar tests/test_gpu_audio_pixel_attn.py applies to the same evaluation."""
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

import attention_track_reference as R  # noqa: E402
from csts_amd import lib as L  # noqa: E402
from csts_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
NAMES = ["grid_6x6", "grid_5x5", "shipped", "wide_17x16"]
GUARD = 64
_DONE = {}


def _guarded(n, dtype):
    """A NaN (or -7) filled buffer with GUARD elements on either side of the n the kernel may write."""
    fill = float("nan") if dtype == torch.float32 else -7
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_untouched(buf):
    edge = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(edge).all()) if buf.dtype == torch.float32 else bool((edge == -7).all())


def _run(name):
    """One launch of every op per case, shared by the tests; the host restatement is computed once."""
    if name not in _DONE:
        Wn, Hh, hd, Tp, h, w, T, S, F, _, _ = R.CASES[name]
        G, HW = Hh + 1, h * w
        case = R.kernel_inputs(name)
        clip = ops.audio_pixel_attn(case["qkv"].to(DEV), case["lse"].to(DEV), (Tp, h, w), Hh, T, S)
        column = clip["column"]
        idx = R.frames_idx(name)
        order, offsets = R.order_offsets(idx, F)
        bufs = {"mixed": _guarded(F * G * HW, torch.float32), "maps": _guarded(F * G * HW, torch.float32),
                "range": _guarded(F * G * 2, torch.float32), "count": _guarded(F, torch.int32)}
        d_order, d_offsets = torch.from_numpy(order).to(DEV), torch.from_numpy(offsets).to(DEV)
        L.check(L.load().csts_attention_track(ops._p(column), ops._p(d_order), ops._p(d_offsets), F, Wn, Hh, Tp, h, w, T, S,
                                              ops._p(bufs["mixed"][1]), ops._p(bufs["maps"][1]), ops._p(bufs["range"][1]),
                                              ops._p(bufs["count"][1]), ops._stream()), "csts_attention_track")
        via_ops = ops.attention_track(column, torch.from_numpy(idx).to(DEV), F, T, S)
        again = ops.attention_rescale(via_ops["mixed"], S, valid=via_ops["count"])
        torch.cuda.synchronize()
        col = column.cpu().numpy()
        mixed, count = R.mean_maps(col, idx, F)
        _DONE[name] = {
            "raw": {"mixed": bufs["mixed"][1].cpu().numpy().reshape(F, G, h, w), "maps": bufs["maps"][1].cpu().numpy().reshape(F, G, h, w),
                    "range": bufs["range"][1].cpu().numpy().reshape(F, G, 2), "count": bufs["count"][1].cpu().numpy()},
            "guards": {k: _guards_untouched(v[0]) for k, v in bufs.items()},
            "ops": {k: v.cpu().numpy() for k, v in via_ops.items()}, "again": {k: v.cpu().numpy() for k, v in again.items()},
            "clip": {k: v.cpu().numpy() for k, v in clip.items()}, "column": col, "idx": idx, "want_mixed": mixed,
            "want_count": count}
    return _DONE[name]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("name", NAMES)
def test_mixed_and_count_equal_the_fp32_restatement_bit_for_bit(name):
    r = _run(name)
    assert r["column"].dtype == np.float32 and float(r["column"].min()) > 0.0
    assert all(r["guards"].values()), r["guards"]
    assert r["raw"]["count"].dtype == np.int32 and np.array_equal(r["raw"]["count"], r["want_count"])
    assert _same_bits(r["raw"]["mixed"], r["want_mixed"])
    for k in ("mixed", "maps", "range", "count"):                  # the lists built on the device give the same bits
        assert _same_bits(r["ops"][k], r["raw"][k]), k


@pytest.mark.parametrize("name", NAMES)
def test_maps_and_range_follow_from_mixed(name):
    r = _run(name)
    S = R.CASES[name][7]
    out, hit = r["raw"], r["want_count"] > 0
    assert 0 < int(hit.sum()) < hit.shape[0]
    assert _same_bits(out["maps"][hit], R.rescale(out["mixed"][hit], out["range"][hit]))
    want = R.lattice_extrema(out["mixed"][hit], S)
    err = float(np.abs(out["range"][hit].astype(np.float64) - want).max())
    bound = 1e-6 * float(np.abs(out["mixed"]).max())
    print(f"attention_track {name}: range off by {err:.3e}, allowed {bound:.3e}")
    assert err <= bound
    # frames no pair lands on
    assert np.array_equal(out["count"][~hit], np.zeros(int((~hit).sum()), dtype=np.int32))
    assert not out["maps"][~hit].any() and not out["mixed"][~hit].any()
    assert np.isnan(out["range"][~hit]).all() and np.isfinite(out["range"][hit]).all()


@pytest.mark.parametrize("name", NAMES)
def test_a_frame_with_one_pair_carries_the_one_clip_maps(name):
    r = _run(name)
    T, F = R.CASES[name][6], R.CASES[name][8]
    seen = 0
    for f, pairs in enumerate(R.pair_lists(r["idx"], F)):
        if len(pairs) != 1:
            continue
        w, j = int(pairs[0]) // T, int(pairs[0]) % T
        assert _same_bits(r["raw"]["maps"][f], r["clip"]["maps"][w, :, j]), (f, w, j)
        assert _same_bits(r["raw"]["range"][f], r["clip"]["range"][w, :, j]), (f, w, j)
        seen += 1
    assert seen >= 2


def test_one_head_is_its_own_mean():
    out = _run("grid_5x5")["raw"]
    assert out["mixed"].shape[1] == 2
    for k in ("mixed", "maps", "range"):
        assert _same_bits(np.ascontiguousarray(out[k][:, 1]), np.ascontiguousarray(out[k][:, 0])), k


@pytest.mark.parametrize("name", NAMES)
def test_rescale_alone_reproduces_maps_and_range(name):
    r = _run(name)
    for k in ("maps", "range"):
        assert _same_bits(r["again"][k], r["ops"][k]), k


def test_rescale_without_valid_takes_every_frame_and_bool_is_int():
    r = _run("grid_6x6")
    S = R.CASES["grid_6x6"][7]
    mixed = torch.from_numpy(r["ops"]["mixed"]).to(DEV)
    count = torch.from_numpy(r["ops"]["count"]).to(DEV)
    every = ops.attention_rescale(mixed, S)
    by_bool = ops.attention_rescale(mixed, S, valid=count > 0)
    hit = r["want_count"] > 0
    assert _same_bits(every["maps"].cpu().numpy()[hit], r["ops"]["maps"][hit])
    assert _same_bits(by_bool["maps"].cpu().numpy(), r["ops"]["maps"]) and _same_bits(by_bool["range"].cpu().numpy(), r["ops"]["range"])
    # an all-zero map without `valid`: extrema (0, 0), maps 0 / 1e-6 = 0
    assert not every["maps"].cpu().numpy()[~hit].any() and not every["range"].cpu().numpy()[~hit].any()


def test_bad_arguments_raise():
    Wn, Hh, hd, Tp, h, w, T, S, F, _, _ = R.CASES["grid_5x5"]
    column = torch.from_numpy(R.host_column("grid_5x5")).to(DEV)
    idx = torch.from_numpy(R.frames_idx("grid_5x5")).to(DEV)
    ops.attention_track(column, idx.int(), F, T, S)                       # int32 frames are fine
    with pytest.raises(ValueError):
        ops.attention_track(column.double(), idx, F, T, S)
    with pytest.raises(ValueError):
        ops.attention_track(column[0], idx, F, T, S)
    with pytest.raises(ValueError):
        ops.attention_track(column, idx[:, :-1], F, T, S)                 # frames_idx is not (Wn, T)
    with pytest.raises(ValueError):
        ops.attention_track(column, idx.float(), F, T, S)
    with pytest.raises(ValueError):
        ops.attention_track(column, idx, 0, T, S)
    with pytest.raises(ValueError):
        ops.attention_track(column, idx, F, T, 0)
    with pytest.raises(ValueError, match="CSTS_AUDIO_PIXEL_MAX_SIDE"):
        ops.attention_track(torch.ones(1, 1, 1, 129, 1, device=DEV), torch.zeros(1, 1, dtype=torch.int64, device=DEV), 2, 1, 16)
    with pytest.raises(L.CstsError):
        ops.attention_track(column.cpu(), idx.cpu(), F, T, S)
    with pytest.raises(L.CstsError):
        ops.attention_track(column.clone().requires_grad_(True), idx, F, T, S)
    mixed = torch.ones(F, Hh + 1, h, w, device=DEV)
    with pytest.raises(ValueError):
        ops.attention_rescale(mixed[0], S)
    with pytest.raises(ValueError):
        ops.attention_rescale(mixed.double(), S)
    with pytest.raises(ValueError):
        ops.attention_rescale(mixed, 0)
    with pytest.raises(ValueError):
        ops.attention_rescale(mixed, S, valid=torch.ones(F + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.attention_rescale(mixed, S, valid=torch.ones(F, device=DEV))
    with pytest.raises(ValueError, match="CSTS_AUDIO_PIXEL_MAX_HW"):
        ops.attention_rescale(torch.ones(1, 1, 65, 64, device=DEV), S)
    # the library's own guard refuses what the binding would let through
    with pytest.raises(L.CstsError):
        L.check(L.load().csts_attention_rescale(ops._p(mixed), None, Hh + 1, F, h, w, S, ops._p(mixed), ops._p(mixed), ops._stream()),
                "csts_attention_rescale")
