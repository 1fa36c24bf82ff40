"""CPU checks of tests/attention_core_reference.py: the float64 restatement of the attention core is the operation (against float64
torch autograd), the device form of frame_of is x // HW, the Python restatement of the host code's plan reaches every kernel
instantiation with the case table, the reduce kernel's second grid-stride trip is unreachable under that plan, and the staircase
cases hold the three kinds of rows the lazy running max of the forward distinguishes."""
import numpy as np
import pytest
import torch

import attention_core_reference as AR

_RUNS = [(n, hd) for n in AR.CASES for hd in AR.CASES[n][4]]


@pytest.mark.parametrize("name,hd", _RUNS, ids=[f"{n}-hd{hd}" for n, hd in _RUNS])
def test_reference_is_the_operation(name, hd):
    """Fed the unrounded float64 O / LSE, the restatement agrees with autograd of softmax(q k^T scale + mask) v to 1e-11 relative
    (of the largest element of each tensor; LSE absolute in units of 1 + |LSE|)."""
    mask = AR.CASES[name][6]
    q, k, v, do = (t.double() for t in AR.operands(name, hd, torch.float32))
    scale = AR.scale_of(hd)
    f = AR.forward(q, k, v, scale, mask)
    b = AR.backward(q, k, v, do, f["O"], f["LSE"], scale, f["z2"])
    g = AR.autograd(q, k, v, do, scale, mask)
    for key, mine in (("O", f["O"]), ("dQ", b["dQ"]), ("dK", b["dK"]), ("dV", b["dV"])):
        assert float((mine - g[key]).abs().max()) <= 1e-11 * float(g[key].abs().max()), key
    assert float(((f["LSE"] - g["LSE"]).abs() / (1 + g["LSE"].abs())).max()) <= 1e-11
    assert float((b["delta"] - (do * g["O"]).sum(-1)).abs().max()) <= 1e-11 * float(b["A_delta"].max())
    assert bool((f["P"].sum(-1) - 1).abs().max() <= 1e-12)
    if mask is not None:                                              # masked keys carry no probability and no gradient path
        live = AR.live_mask(mask, q.shape[2], k.shape[2])
        assert float(f["P"][..., ~live].abs().max()) == 0.0 if (~live).any() else True


def test_magnitudes_bound_the_outputs():
    r = AR.reference("ragged_both", 96, "bf16")
    for key in ("O", "dQ", "dK", "dV", "delta"):
        assert bool((r[key].abs() <= r["A_" + key] * (1 + 1e-12)).all()), key
    z = AR.reference("zero_head", 96, "bf16")
    for key in ("dQ", "dK", "dV"):
        assert float(z["A_" + key][:, 1].abs().max()) == 0.0 and float(z[key][:, 1].abs().max()) == 0.0
    assert float(z["A_delta"][:, 1].max()) == 0.0


@pytest.mark.parametrize("HW", list(range(1, 65)) + [49, 196, 255, 256, 257, 1023, 1024, 1025, 3136, 4095, 4096])
def test_frame_of_float_form_is_floor_division(HW):
    x = np.arange(1 << 20, dtype=np.int64)
    assert np.array_equal(AR.frame_of_f32(x, HW), (x // HW).astype(np.int32))


def test_mask_2x41_needs_the_half():
    """Without the + 0.5f the device form puts token 41 of HW = 41 into frame 0: the case mask_2x41 holds that token."""
    x = np.arange(84, dtype=np.int64)
    inv = np.float32(1.0) / np.float32(41)
    assert (x.astype(np.float32) * inv).astype(np.int32)[41] == 0 and AR.frame_of_f32(x, 41)[41] == 1
    assert AR.CASES["mask_2x41"][6] == (2, 41)


def test_frame_ids():
    assert AR.frame_ids(3, 2).tolist() == [0, 0, 1, 1, 2, 2, 0, 1, 2]
    live = AR.live_mask((5, 1), 10, 10)
    assert live.sum(-1).tolist() == [2] * 10                         # (5, 1): two live keys per row


# ------------------------------------------------------------------------------------------------------------ the plan
DEFAULT = AR.env_of({})


def _plan(name, hd, dk, env=DEFAULT):
    B, H, Nq, Nk, _, _, mask, _ = AR.CASES[name]
    return AR.plan(B, H, Nq, Nk, hd, dk == "h16", mask is not None, env)


def test_env_restated():
    assert DEFAULT == {"fwd_fast": True, "dkv_fast": True, "fused": True, "dq": -1}
    e = AR.env_of(AR.CHILD_ENV["generic"])
    assert e == {"fwd_fast": False, "dkv_fast": False, "fused": False, "dq": 0}
    assert AR.env_of({"CSTS_ATTN_DQ_FAST": "4"})["dq"] == 4 and AR.env_of({"CSTS_ATTN_FUSED_BWD": "1"})["fused"]


def test_the_case_table_takes_the_paths_it_names():
    """The splits, chunks and kernels the table of the cases promises."""
    p = _plan("ragged_both", 96, "h16")
    assert (p["fwd"], p["dq"], p["dkv"], p["nsplit"], p["q_chunk"]) == ("attn_fwd_kernel<96,false>", "attn_dq_kernel<96,false>", "attn_dkv_kernel<96,false,true>", 2, 192)
    p = _plan("whole_fast", 96, "h16")
    assert (p["fwd"], p["dq"], p["dkv"], p["nsplit"], p["q_chunk"]) == ("attn_fwd_fast_kernel", "attn_dq_fast_kernel<2>", "attn_dkv_kernel<96,false,false>", 2, 384)
    p = _plan("whole_single", 96, "h16")
    assert (p["dkv"], p["nsplit"], p["ws"]) == ("attn_dkv_kernel<96,false,false>", 1, 16)
    assert _plan("whole_single", 96, "h16", AR.env_of(AR.CHILD_ENV["dq4"]))["dq"] == "attn_dq_fast_kernel<4>"
    assert _plan("dq4_three_tiles", 96, "h16", AR.env_of(AR.CHILD_ENV["dq4"]))["dq"] == "attn_dq_fast_kernel<4>"
    p = _plan("fast_ragged_q", 96, "h16")
    assert (p["fwd"], p["dq"], p["dkv"]) == ("attn_fwd_fast_kernel", "attn_dq_fast_kernel<2>", "attn_dkv_kernel<96,false,true>")
    p = _plan("hd192_whole", 192, "h16")
    assert (p["dkv"], p["nsplit"], p["q_chunk"]) == ("attn_dkv_kernel<192,false,false>", 2, 96)
    p = _plan("hd192_ragged", 192, "h16")
    assert (p["dkv"], p["nsplit"], p["q_chunk"]) == ("attn_dkv_kernel<192,false,true>", 2, 96)
    assert _plan("hd192_ragged", 192, "f32")["dkv"] == "attn_dkv_kernel<192,true,true>"
    for name, ns, chunk in (("fused_ragged", 5, 256), ("fused_whole", 4, 256), ("fused_tiny_kv", 5, 256), ("fused_kv33", 4, 256), ("fused_single_split", 1, 1024)):
        p = _plan(name, 96, "h16")
        assert (p["path"], p["nsplit"], p["q_chunk"]) == ("one-pass", ns, chunk), name
        g = _plan(name, 96, "h16", AR.env_of(AR.CHILD_ENV["generic"]))
        assert g["path"] == "two-kernel" and g["dkv"] == "attn_dkv_kernel<96,false,true>"
    assert 1100 - 4 * 256 == 76 and 1030 - 4 * 256 == 6
    p = _plan("mask_4x64", 96, "h16")
    assert (p["dkv"], p["nsplit"], p["q_chunk"]) == ("attn_dkv_kernel<96,false,true>", 2, 192)
    B, H, Nq, Nk, hd = AR.PROBS_CAP
    assert B * H * Nq * Nk == 1228800 > 4096 * 256


def test_every_instantiation_is_reached():
    """In-process cases under the default environment plus the three children (each with the environment of its process) reach
    every kernel instantiation behind csts_attn_fwd / _bwd / _probs."""
    got = AR.reached(AR.IN_PROCESS, DEFAULT)
    for mode, names in AR.CHILD_CASES.items():
        got |= AR.reached(names, AR.env_of(AR.CHILD_ENV[mode]), half_only=True)
    assert got == set(AR.INSTANTIATIONS), (set(AR.INSTANTIATIONS) - got, got - set(AR.INSTANTIATIONS))
    assert len(AR.INSTANTIATIONS) == 5 + 6 + 6 + 2 + 2           # forward, dQ, dK/dV, one-pass (split / direct), reduce and probs
    # what each child adds: the generic forward / dQ at whole tiles, the 128-key dQ, nothing new in kind for fp16 (another library)
    gen = AR.reached(AR.CHILD_CASES["generic"], AR.env_of(AR.CHILD_ENV["generic"]), half_only=True)
    assert gen == {"attn_fwd_kernel<96,false>", "attn_dq_kernel<96,false>", "attn_dkv_kernel<96,false,true>", "attn_dkv_reduce_kernel"}
    assert "attn_dq_fast_kernel<4>" not in AR.reached(AR.IN_PROCESS, DEFAULT)


def test_reduce_second_trip_is_unreachable():
    """attn_dkv_reduce_kernel runs min(cdiv(total8, 256), 4096) workgroups: a second grid-stride trip needs 2 B H Nk hd / 8 >
    4096 * 256, that is B H Nk hd > 4,194,304.  It runs only when nsplit > 1.  Two-kernel path: nsplit > 1 needs want >= 2, so
    cdiv(Nk, 128) B H <= 128 and B H Nk hd <= 128 * 128 * 192 = 16384 * 192 = 3,145,728.  One-pass path: B H <= 128 and Nk <= 128, hd
    96: <= 1,572,864.  The plan is swept over its variables to hold both bounds; a plan that makes the trip reachable fails here."""
    limit = 4096 * 256 * 8 // 2
    assert 16384 * 192 < limit and 128 * 128 * 96 == 1572864 < limit
    worst = {"two-kernel": 0, "one-pass": 0}
    for env in (DEFAULT, AR.env_of(AR.CHILD_ENV["generic"])):
        for h16 in (False, True):
            for hd in (96, 192):
                for BH in (1, 2, 3, 7, 64, 127, 128, 129, 256, 257):
                    for Nk in (1, 8, 127, 128, 129, 1024, 16384, 16385, 1 << 17):
                        for Nq in (1, 127, 1024, 4096, 1 << 17):
                            p = AR.plan(1, BH, Nq, Nk, hd, h16, False, env)
                            if p["reduce"]:
                                worst[p["path"]] = max(worst[p["path"]], BH * Nk * hd)
    assert 0 < worst["two-kernel"] <= 16384 * 192 and 0 < worst["one-pass"] <= 1572864, worst


# ------------------------------------------------------------------------------------------------------------ the staircase
@pytest.mark.parametrize("name", ["staircase", "staircase20"])
@pytest.mark.parametrize("store", ["f32", "bf16", "fp16"])
def test_staircase_rows(name, store):
    """From the float64 scores of the rounded operands: each variant holds rows that rescale after tile 0, rows that go two tiles
    in a row without a rescale although their max grew, and rows that never rescale after tile 0."""
    r = AR.reference(name, 96, store)
    tiles = r["z2"][0, 0].reshape(128, 8, 64).amax(-1)                # (Nq, 8 tiles of 64 keys)
    kinds = np.array([AR.rescale_kinds(row.tolist()) for row in tiles])
    assert kinds[:, 0].sum() >= 16 and kinds[:, 1].sum() >= 16 and kinds[:, 2].sum() >= 16, kinds.sum(0)
    rises = (tiles[0::3, 1:] - tiles[0::3, :-1]).mean()
    assert abs(float(rises) - AR.STAIR_RISE[name]) < 1.0
    if name == "staircase20":                                         # the fast rows rescale at every tile; falling rows underflow
        assert all(all(row[1:] > row[:-1] + 8) for row in tiles[0::3].numpy())
        assert float(r["P_in"][0, 0, 2::3, 448:].max()) < 2.0 ** -126      # below the fp32 normal range: 0 on the device


def test_big_variant_keeps_ds_representable():
    for name in AR.CHILD_CASES["fp16"]:
        for hd in AR.CASES[name][4]:
            r = AR.reference(name, hd, "fp16", "_big")
            assert r["A_dS_max"] < 2 ** 15 and r["do_scale"] >= 1.0, (name, r["do_scale"])
            assert 1e4 < float(r["v_fwd"].abs().max()) <= 3.2e4 and float(r["O"].abs().max()) < 65504
