"""CPU checks of tests/attention_core_reference.py: the float64 restatement of the attention core is the operation (against float64
torch autograd), the device form of frame_of is x // HW, the Python restatement of the host code's plan reaches every kernel
instantiation with the case table, the reduce kernel's second grid-stride trip is unreachable under that plan, the built library's
own route (csts_attn_route, csts_attn_bwd_workspace) is that restatement in every environment, and the staircase cases hold the
three kinds of rows the lazy running max of the forward distinguishes."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_core_reference as AR
import attention_route_worker as AW
from conftest import ROOT
from csts_amd import lib as L

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


# ------------------------------------------------------------------------------------------------------------ the library's route
# What the plan tests above prove about the restatement holds for the library only while the two agree: the built library is asked
# (csts_attn_route, csts_attn_bwd_workspace; host-only, no GPU) for every run of the case table, PROBS_CAP and a sweep that
# hits every threshold of the plan on both sides, in every environment the suite runs attention in and with each switch alone.
_OFF = {f"{s[10:].lower()}_off": {s: "0"} for s in AR.SWITCHES}
ROUTE_ENV = {"generic": AR.CHILD_ENV["generic"], "dq4": AR.CHILD_ENV["dq4"], **_OFF, "fp16": {"CSTS_HALF": "fp16"}}


def test_route_problems_straddle_the_thresholds():
    assert set(_OFF) == {"fwd_fast_off", "dq_fast_off", "dkv_fast_off", "fused_bwd_off"}
    assert {255, 256, 1023, 1024} <= set(AW.SWEEP_NQ) and {64, 65, 128, 129, 192} <= set(AW.SWEEP_NK)
    probs = AW.problems()
    assert len(probs) == len(AR.runs(AR.CASES)) + 1 + 2 * 2 * 10 * 12 * 8 and any(p[6] is not None for p in probs)


def test_library_route_is_the_restatement():
    """The default environment, in this process."""
    n, bad = AW.mismatches(L.load(), AR.env_of())
    assert n > 3800 and not bad, (len(bad), bad[:3])


@pytest.mark.parametrize("mode", list(ROUTE_ENV))
def test_library_route_is_the_restatement_in_a_child(mode, tmp_path):
    """Every other environment in a host-only process of its own: the switches are read once per process, and the fp16 run loads
    the other library."""
    base = {k: v for k, v in os.environ.items() if k not in ("CSTS_HALF",) + AR.SWITCHES}
    out = tmp_path / "route.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attention_route_worker.py"), str(out)], cwd=ROOT,
                       env={**base, **ROUTE_ENV[mode]}, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    r = json.load(open(out))
    assert r["env"] == AR.env_of(ROUTE_ENV[mode]) and r["half_kind"] == (1 if mode == "fp16" else 0)
    assert r["checked"] > 3800 and r["n_bad"] == 0, (r["n_bad"], r["bad"])


def test_route_query_refuses_what_the_workspace_query_refuses():
    lib = L.load()
    for kw in ({"B": 0}, {"H": 0}, {"Nq": 0}, {"Nk": 0}, {"B": -1}, {"Nk": -5}, {"head_dim": 64}, {"head_dim": 0}):
        a = AW.args_of(2, 2, 300, 100, 96, True, None)
        for k, v in kw.items():
            setattr(a, k, v)
        assert AW.route(lib, a)[0] == -1 and b"csts_attn_route" in lib.csts_last_error(), kw
        assert lib.csts_attn_bwd_workspace(C.byref(a)) == 0, kw
    assert AW.route(lib, None)[0] == -1 and lib.csts_attn_bwd_workspace(None) == 0
    ok = AW.args_of(2, 2, 300, 100, 96, True, None)
    assert AW.route(lib, ok)[0] == 0 and lib.csts_attn_bwd_workspace(C.byref(ok)) == 2 * 2 * 4 * 100 * 96 * 4


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
