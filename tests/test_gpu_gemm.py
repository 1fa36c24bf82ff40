"""The GEMM kernels of csts_amd/csrc/gemm.hip, gemm4.hip and gemm5.hip, element by element against fp64 (tests/gemm_reference.py),
through raw csts_gemm calls on operands between guard bands (tests/gemm_raw.py): every operand a window of a wider buffer (leading
dimensions = extent + pad), inputs NaN outside their extent, outputs (C, aux, colsum, the split-K workspace) pre-filled with NaN
between sentinel guards.  After a call every owned element is finite, every sentinel intact, what the call was not to write still
holds its pre-fill, and the kernel csts_gemm_kernel_name gives for the real arguments is the one the case names.

Bars (u = 2^-24; u_out = 0 / 2^-8 / 2^-11 for fp32 / bf16 / fp16 storage, + 2^-25 for fp16; derivations in tests/gemm_reference.py):
  C       |err| <= k u S + 2 u P + F + u_out |C64|,  S = (|A|.|B| + |bias|) |slope| |scale| + |residual| (slope 1 without an activation),
          P = |act| |scale| with GELU / DGELU, else 0: the two roundings behind the activation, DERIVED, not scaled by the measured k
  aux     |err| <= k u S_pre + u_out |pre64|
          k = min(c_derived, BARS k): c_derived = 2 (K + nsplit) + 3 (+ 1 fp32 mode, + 14 res_up) DERIVED; BARS k measured
  F       gelu_fast 0.5 |x| E, dgelu_fast (0.5 E + |h| pdf(h) c_f u) |pre|, E = 1.5e-7 + c_f u; libm forms c_f u (x |pre|); absolute.
          1.5e-7 is the bound common.h states (DERIVED there); c_f measured (BARS cf)
  colsum  |err| <= 2 (K + nsplit) u colsum|A|                                                   DERIVED   worst 0.06
  `exact` value sets: C (without an activation), aux and colsum equal C64 rounded once to the storage type          BIT-EQUAL
  finishing pass vs its exact-order fp32 emulation; a second call; gemm4 FORM 5 and gemm5 vs gemm2                  BIT-EQUAL
Every owned element is compared; no floor but the fp16 subnormal term.  Values: plain = randn; offset = randn + 1.5 for A and B with
bias and residual (1 + K / 10) randn; exact = small integers (tests/gemm_reference.py); GELU cases take plain for their random set (offset
pre-activations all sit on the linear branch).  Smallest S per value set over the cases without an activation (every test prints
it): plain 0.086 and offset 0.077 at K = 1; 2.5e-5 / 3.4e-3 on the rows whose row scale is 0 (S = |residual| there, on purpose);
exact 0 (an all-zero product at K = 1, a zero scale over a zero residual: the result must then be exactly 0).

Which test runs which kernel (all 135 instantiations; tests/test_gemm_reference_host.py holds the tables to that list on the host):
  test_gemm_tiny_kernel   gemm_tiny_kernel<layout, wave>: 6.  K 1, 16 (thread) / 17, 64, 65 (wave), bias or none, odd ld, A off by one
  test_gemm_kernel        gemm_kernel<A_KC, B_KC, F32>: 6.  (1,1,1) (65,97,40) (128,128,32) (129,130,33); scalar and vector staging; every
                          epilogue; res_up 2 x 2 x 4; atomic and deterministic split_k = 3 at K = 40 (2 slabs) and 200 (3)
  test_gemm2_kernel       gemm2_kernel<A_KC, B_KC, A_F32, B_F32, MT, 2>: 21.  Tile rows 64 / 128 / 256 forced, M = rows + 24, N = 136,
                          K 8 / 64 / 72 / 128; colsum unsplit and deterministic; res_row_mod 40 / 72; rows_per_scale 1 / 100 / M with a
                          zero scale; res_up; the whole-line residual epilogue (res_lines); the DGELU and GELU fast paths; the automatic tile
  test_gemm3_kernel       gemm3_kernel<MT, S>: 8, algo 300 + 10 MT + S.  K 16 / 48 / 64 / 96 / 64 S / 64 S + 16, M 40 and 64 MT + 8; the
                          residual-stream epilogue of <1, S>; algo 1312: 264 tiles on 256 workgroups
  test_gemm4_kernel       gemm4_kernel<WM, MT, NT, S, FORM, NP>: 72, algo 400 + variant.  Forms 1 - 5 at K = 64 and 64 (S + 1); FORM 2 with
                          aux NULL; FORM 5 with / without bias, rows_per_scale 32 and 100; FORM 0 ragged and with the epilogues the forms
                          leave to it; the producer-wave variants 83, 84; algo 1400 + variant: 257 tiles on 256 workgroups per tile shape
  test_gemm5_kernel       gemm5_kernel<KCH, NB, W, FORM>: 22, algo 500 / 503 / 506.  M 32 and 96; one pass of the grid + 32 rows per
                          (KCH, NB, W); N = 768, K = 96 form 3: 8192 + 32 and 16384 + 32 rows (second and third units of one wave); every form-3
                          kernel at M = 160 with rows_per_scale 32 and 64
  test_splitk_finish_kernel   splitk_finish_kernel<VEC, SL>: 6 (VEC 4 / 1 x SL 1 / 4 / 16) behind gemm_kernel<true, true, true>
  test_switch_reached_kernels a child with CSTS_GEMM4_T64=3, CSTS_GEMM5_K384=1, CSTS_GEMM5_WIDE192=1, CSTS_GEMM_RES_LINES=0, algo 0.
                          (RES_LINES is a compile-time choice of gemm2_kernel since -DCSTS_GEMM_RES_OLD: the variable selects nothing
                          in this build, the case runs the whole-line form and must give the same name and hold the same bars.)
  test_fp16_library       libcsts_hip_f16.so: an exact and a random case per family, every gemm5 form, gemm4 forms 0, 2, 4, 5, big, subnormal

No kernel changed: the suite found no bug.  The fp32 constants of the six families lie between 2.6 and 7.5 (all on offset values),
every `exact` case is bit-equal, and every documented "same arithmetic" pair has equal bits.

Mutation check (scratch builds loaded through CSTS_HIP_LIB, one arithmetic-only change each: no new address, no longer loop), run
on MI355X against the tests of this file that use the bf16 library.  Failing tests of the 1005 of this file, all six run:
  32  (a) gemm3's k-tail one sub-step short for K % 64 = 32 and 48 (test_gemm3_kernel: every K = 48 and K = 96 case of the 8 kernels)
  45  (b) gemm4 FORM 2 takes the bias of lane ^ 1's column (test_gemm4_kernel 44: every form-2 case of the 11 variants;
          test_switch_reached_kernels 1)
  12  (c) gemm5 does not clear the accumulators before a wave's second unit (test_gemm5_kernel: the 12 grid-pass cases -- `exact` row
          scales are non-zero unless a case sets scale_zero, so no second unit is multiplied away)
  40  (d) gemm2 adds the residual before the row scale (test_gemm2_kernel 30, the gemm4 / gemm5 bit comparisons 9, the switch child 1)
   3  (e) SL = 16 of the finishing pass leaves out its last lane (test_splitk_finish_kernel: the three 17-slab cases)
  97  (f) one coefficient of erf_poly_times_exp changed in the fifth digit (0.254829592 -> 0.254839592; shared by gelu_fast and
          dgelu_fast; test_gemm2_kernel 5, test_gemm3_kernel 20, test_gemm4_kernel 55, test_gemm5_kernel 17): the DGELU cases with a
          16-bit aux, and the GELU cases with fp32 C beside a 16-bit aux on plain values -- a 16-bit C hides a 1e-5 error of
          gelu_fast under its own rounding, whatever the test (0.5 |x| 1e-5 against 2^-9 |gelu(x)|)
Of these, the GEMM tests of tests/test_gpu_ops.py (whole-tensor rel-L2 at 6e-3 / 1e-4 / 2e-2 against fp32 torch), judged from their
shapes and tolerances, not run: (a) they would see (K = 96 and 160 of test_gemm_nt_persistent_kernel have a two-sub-step tail: 16 of
96 products missing is a rel-L2 of 0.4); (b) likely (a wrong O(1) bias against pre-activations of O(sqrt K) is above 6e-3); (d) yes
(1e-4 with a row scale); (c) no: no shape there gives a wave a second unit (16384 x 768 x 96 is exactly one pass); (e) no: their
split-K cases ask for 3 slabs; (f) no: 1e-5 is far inside 6e-3.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected everywhere, run only on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import lib as L                    # noqa: E402
import gemm_raw as R                             # noqa: E402
import gemm_reference as GR                      # noqa: E402
import test_gemm_reference_host as HOST          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")

# Measured bars, about 4x the worst value seen on MI355X against fp64 over every case of this file and of the two child processes (the
# measured value in the comment).  k: per kernel family and storage kind of the tensor the bar is about (C, or aux); cf: per function.
BARS = {
    "k": {
        "gemm_tiny": {"f32": 10.3},                               # 2.57
        "gemm": {"f32": 28.2, "bf16": 0.52, "fp16": 0.5},         # 7.05, 0.13, 0.00
        "gemm2": {"f32": 20.3, "bf16": 0.5, "fp16": 0.5},         # 5.08, 0.00, 0.11
        "gemm3": {"f32": 27.3, "bf16": 0.52, "fp16": 0.5},        # 6.82, 0.13, 0.07
        "gemm4": {"f32": 29.8, "bf16": 1.4, "fp16": 0.5},         # 7.45, 0.34, 0.11
        "gemm5": {"f32": 26.3, "bf16": 2.2, "fp16": 0.5},         # 6.58, 0.55 (see below), 0.07
    },
    "cf": {"gelu_fast": 1.0, "dgelu_fast": 2.3, "gelu_libm": 5.6, "dgelu_libm": 3.1},   # 0.00, 0.57 (fp16 library), 1.38, 0.76
}
# Every fp32 worst is an `offset` case (all products positive: the roundings of the partial sums do not cancel), K = 16 .. 320, and the
# families lie within 2.6 .. 7.5 of each other: no outlier to explain.  A 16-bit C or aux hides the accumulation under u_out |ref|;
# the 0.55 of gemm5 is aux and C at one element of the 12320 x 384 x 384 GELU case where the products cancel to pre = -9.3e-5 under
# S_pre = 261: the fp32 sum is 8e-6 off, a tenth of the value, and no 16-bit rounding is large enough to hide it.
# 0.5 is the floor of those constants (half a rounding of S), and 1.0 that of gelu_fast, whose error never left 0.5 |x| 1.5e-7.


def _hold(cid, expect, r):
    """Print the figures, then assert every flag, the kernel name and every bar."""
    print(f"\n[{cid}] {r['kernel']}  " + "  ".join(f"{k} {r[k]:.3e}" for k in ("k", "k_aux", "cf", "colsum_ratio", "min_S") if k in r)
          + f"  c_derived {r['c_derived']}")
    bad = R.misses(r, BARS, expect)
    assert not bad, (cid, bad)


def _ids(table):
    return [e[0] for e in table]


def test_host_copies_of_the_fp32_bars():
    """tests/test_gemm_reference_host.py proves on the CPU that wrong kernels miss these bars by a factor of 4; it cannot import this
    module where there is no GPU, so it carries copies."""
    assert HOST.K_F32 == {f: v["f32"] for f, v in BARS["k"].items()} and HOST.CF == BARS["cf"]


# ------------------------------------------------------------------------------------- one parametrised test per family
_TINY, _GENERIC, _G2, _G3, _G4, _G5 = (R.TABLES[t]() for t in ("tiny", "generic", "gemm2", "gemm3", "gemm4", "gemm5"))


@pytest.mark.parametrize("cid,expect,c", _TINY, ids=_ids(_TINY))
def test_gemm_tiny_kernel(cid, expect, c):
    _hold(cid, expect, R.run(c, DEV, BARS))


@pytest.mark.parametrize("cid,expect,c", _GENERIC, ids=_ids(_GENERIC))
def test_gemm_kernel(cid, expect, c):
    _hold(cid, expect, R.run(c, DEV, BARS))


@pytest.mark.parametrize("cid,expect,c", _G2, ids=_ids(_G2))
def test_gemm2_kernel(cid, expect, c):
    _hold(cid, expect, R.run(c, DEV, BARS))


@pytest.mark.parametrize("cid,expect,c", _G3, ids=_ids(_G3))
def test_gemm3_kernel(cid, expect, c):
    _hold(cid, expect, R.run(c, DEV, BARS))


@pytest.mark.parametrize("cid,expect,c", _G4, ids=_ids(_G4))
def test_gemm4_kernel(cid, expect, c):
    _hold(cid, expect, R.run(c, DEV, BARS))


@pytest.mark.parametrize("cid,expect,c", _G5, ids=_ids(_G5))
def test_gemm5_kernel(cid, expect, c):
    _hold(cid, expect, R.run(c, DEV, BARS))


# ------------------------------------------------------------------------------------- the finishing pass of deterministic split-K
_FIN = R.finish_cases()


@pytest.mark.parametrize("cid,expect,c", _FIN, ids=_ids(_FIN))
def test_splitk_finish_kernel(cid, expect, c):
    """The slabs the main kernel left in the workspace, summed in the order of splitk_finish_kernel<VEC, SL> by an fp32 emulation
    (lane l takes slabs l, l + SL, ...; the lanes are folded in order; then the bias): C must have those bits, and a second call
    must give them again."""
    keep = {}
    r = R.run(c, DEV, BARS, keep=keep, twice=True)
    vec, sl = GR.finish_form(c, r["nsplit"])
    want = GR.finish_emulation(keep["ws"], r["nsplit"], sl, keep["bias"], keep["C"].dtype)
    print(f"\n[{cid}] VEC {vec} SL {sl} slabs {r['nsplit']}")
    assert torch.equal(want, keep["C"]), (cid, int((want != keep["C"]).sum()))
    assert r["twice_equal"] is True
    _hold(cid, expect, r)


def test_every_finishing_form_ran():
    forms = sorted(GR.finish_form(c, GR.split_plan(c, n)[1]) for _, n, c in _FIN[:6])
    assert forms == R.FINISH_FORMS


# ------------------------------------------------------------------------------------- routes documented to share their arithmetic
def _bits(c, **kw):
    keep = {}
    r = R.run(dict(c, **kw), DEV, BARS, keep=keep)
    return r["kernel"], keep["C"]


@pytest.mark.parametrize("variant", [33, 63, 73, 83])
@pytest.mark.parametrize("kind", ["plain", "offset"])
def test_gemm4_fp32_residual_form_gives_gemm2_bits(variant, kind):
    """gemm4 FORM 5 "Same arithmetic order as gemm2: bit-identical" (gemm4.hip) -- the claim of test_gemm4_fp32_residual_form in
    tests/test_gpu_ops.py, here at two tiles of each shape, three k-tiles, with a bias and a row scale every 100 rows."""
    BM, BN = R.g4_tile(variant)
    c = GR.case("NT", 2 * BM, 2 * BN, 192, bias=True, rps=100, kind=kind, seed=variant, **R.RES)
    n4, c4 = _bits(c, algo=400 + variant)
    n2, c2 = _bits(c, tile_rows=128)
    assert n4 == R.name_gemm4(variant, 5) and n2 == R.name_gemm2("NT", "h16", "h16", 128)
    assert torch.equal(c4, c2), int((c4 != c2).sum())


@pytest.mark.parametrize("form", [0, 3, 4])
def test_gemm5_gives_gemm2_bits(form):
    """gemm5: "k ascending: the arithmetic order of gemm2_kernel", "Same epilogue arithmetic, term for term, as gemm2_kernel"
    (gemm5.hip) -- the forms without an activation."""
    c = GR.case("NT", 96, 192, 192, kind="plain", seed=form, **R._g5_form_kw(form, 0))
    n5, c5 = _bits(c, algo=503)
    n2, c2 = _bits(c, tile_rows=64)
    assert n5 == R.name_gemm5(2, 3, 8, form) and n2 == R.name_gemm2("NT", "h16", "h16", 64)
    assert torch.equal(c5, c2), int((c5 != c2).sum())


# ------------------------------------------------------------------------------------- child processes
def _child(mode, tmp_path_factory, extra_env):
    path = tmp_path_factory.mktemp("gemm") / f"{mode}.json"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSTS_HALF") and not k.startswith("CSTS_GEMM")}
    env.update(extra_env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm_worker.py"), mode, str(path), json.dumps(BARS)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.load(open(path))


@pytest.fixture(scope="module")
def fp16_child(tmp_path_factory):
    """One child process on libcsts_hip_f16.so, with a timeout."""
    if not os.path.exists(L._PATHS["fp16"]):
        pytest.skip(f"{L._PATHS['fp16']} is not built (make -C csts_amd/csrc f16)")
    return _child("fp16", tmp_path_factory, {})


_FP16 = R.fp16_cases()


@pytest.mark.parametrize("cid,expect,c", _FP16, ids=_ids(_FP16))
def test_fp16_library(fp16_child, cid, expect, c):
    """libcsts_hip_f16.so: IEEE-half operands (the bars of 16-bit outputs carry + 2^-25); `big`: max |C64| in (1.5e4, 3e4], `subnormal`:
    in (2^-16, 2^-15]."""
    assert fp16_child["half_kind"] == 1
    _hold(cid, expect, fp16_child[cid])


@pytest.fixture(scope="module")
def switch_child(tmp_path_factory):
    """One fresh child process with the library's switches set."""
    return _child("switch", tmp_path_factory, R.SWITCH_ENV)


_SWITCH = R.switch_cases()


@pytest.mark.parametrize("cid,expect,c", _SWITCH, ids=_ids(_SWITCH))
def test_switch_reached_kernels(switch_child, cid, expect, c):
    """CSTS_GEMM4_T64=3, CSTS_GEMM5_K384=1, CSTS_GEMM5_WIDE192=1, CSTS_GEMM_RES_LINES=0: what algo 0 routes to then, by name, held
    to the same bars."""
    assert switch_child["half_kind"] == 0
    _hold(cid, expect, switch_child[cid])
