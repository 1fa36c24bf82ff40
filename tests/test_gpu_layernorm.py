"""The LayerNorm kernels and the row reducers of csts_amd/csrc/norm.hip, element by element against fp64 (tests/layernorm_reference.py),
through raw C-ABI calls on operands between guard bands (tests/layernorm_raw.py): csts_layernorm_fwd / _fwd_add / _bwd / _bwd_ex /
_bwd2, csts_reduce_rows / _batched / _wide.  Every output is pre-filled with NaN between sentinel guards, every input is NaN
outside its own extent: after a call every owned element is finite, nothing else was touched, nothing foreign was read.

Bars (u = 2^-24; u_out = 0 / 2^-8 / 2^-11 for fp32 / bf16 / fp16 storage; derivations in tests/layernorm_reference.py):
  mean                 |err| <= (C + 1) u mean_c|x|                                                   DERIVED   worst 0.36 (C 7)
  16-bit copy of dx    |copy - dx_stored scale| <= (u + u_out)(1 + u) |dx_stored scale| (+ 2^-25 fp16)  DERIVED   worst 0.996
  reducers vs fp64     |err| <= (ceil(nrows / RL) + RL + 1) u |scale| sum_i |ws_ij|; wide: (nrows + 1)   DERIVED   worst 0.64
  reducers vs the exact-order fp32 emulation, sum_out vs (x + a).to(dtype), deferred vs not, bwd2 vs bwd   BIT-EQUAL
  rstd per row, relative; y, dx per element: |err| <= K u S + u_out |ref|; dgamma, dbeta: |err| <= K u S   measured: BARS below
fp16 storage adds 2^-25 (half its smallest subnormal) to the bar of every 16-bit output.  The derived ratios |err| / bar must be
<= 1; the copy reaches 0.996 because its bar IS the rounding of a 16-bit value at the bottom of a binade.

Values: plain = 2 randn, offset = randn + 64 (separates one-pass from two-pass statistics: tests/test_layernorm_reference_host.py),
flat = 3 + 1e-4 randn with one constant row; gamma = 1 + 0.3 randn, beta = 0.3 randn.  The backward kernels are handed the fp64
mean and rstd of the x they read, rounded to fp32.  Smallest row variance per case (every test prints it): plain / offset rows
0.032 (C 7), 0.036 (C 8, 16421 rows), 0.12 (C 8, 16), >= 0.37 at C >= 24 -- no such row is near zero; exactly 0 at C = 1 (a row
of one element) and in test_flat_rows (1e-8 and the constant row, on purpose); 2.3e-11 in the fp16 subnormal set (on purpose).

Which test runs which kernel.  ln_fwd_kernel / ln_bwd_kernel <W, GL, NCH, R, ...> are one template per direction: W = 8 channels
per lane and chunk (C % 8 == 0, every operand 16-byte aligned) or W = 1 (everything else, a whole wave per row).  Every form runs
with XF32 / YF32 resp. DYF32 / XF32 both ways: the dtype pairs are dealt over the rows.
  W = 1:  <1,64,2,4>   C 1, 7, 63, 65, 100   <1,64,3,4>  C 129, 191   <1,64,6,2>  C 250, 383   <1,64,12,1>  C 500, 767
      test_small_forward / _backward; at C 96 / 192 / 384 / 768 through a misaligned operand: test_scalar_kernels_at_model_widths
  W = 8:  <8,16,1>  C 8, 16, 24, 40, 96, 128 (1, 2, 3, 5, 12, 16 of 16 lanes active)   <8,32,1>  C 136, 192, 256 (17, 24, 32 of 32)
      <8,64,1>  C 264, 384, 512 (33, 48, 64 of 64)   <8,64,2>  C 520, 768 (second chunk: 1, 32 lanes)   (R: 2 forward, 1 backward)
      test_small_forward / _backward
  segment 1 of both roles of the backward kernel (blockIdx.y == 1, gamma1, the workspace offset): test_bwd2
  reduce_rows_kernel<2> nrows 1, 2, 3, 8   <8> 9, 63, 64   <32> 65, 129, 515: test_reduce_rows; as the second stage of a deferred
      backward (3, 10, 66, 512 partial rows): test_bwd_deferred_second_stage
  reduce_rows_batched_kernel: test_reduce_rows_batched     reduce_rows_wide_kernel: test_reduce_rows_wide*
  libcsts_hip_f16.so, all of the LayerNorm cases above but the trips: test_fp16_library
Grid-stride trips (computed grid | cap): forward W = 8 C 96, 131107 rows: 4098 | 4096 workgroups of 32 rows; C 768, 32777 rows:
4098 | 4096 of 8 rows; forward W = 1 C 100, 65543 rows: 4097 | 4096 of 16 rows.  Backward (cap 512): C 96, 16421 rows: 514
workgroups of 32 rows; C 192, 16403: 513 of 16; C 384, 8201: 513 of 8; C 768, 4105: 514 of 8; W = 1 C 100, 16389: 513 of 32;
C 383, 8195: 513 of 16; C 767, 4099: 513 of 8.  C 192 with 8211 rows and C 384 with 4105 launch 257 workgroups, not capped, and
still take two trips (see test_grid_stride_backward).  csts_reduce_rows_wide: 4097 | 4096 workgroups.

A bug these tests found, fixed in norm.hip: csts_layernorm_fwd_add with 16-bit x took the statistics of the unrounded fp32 sum while
storing the rounded one (test_fwd_add_16bit_sum_consumed_by_backward).  The model's residual stream is fp32: its results are unchanged.

Mutation check (scratch builds of norm.hip loaded through CSTS_HIP_LIB, one arithmetic-only change each, no new address and no
longer loop).  The counts were taken while each role (W = 8, W = 1) was a kernel text of its own: a mutant changed the one role
it names.  Of the 108 tests here that run the bf16 library, on MI355X, each mutant fails:
  20  (a) the W = 8 role of ln_fwd_kernel computes the variance as E[x^2] - mean^2
          (test_small_forward 14: every W = 8 width; test_flat_rows 3, test_grid_stride_forward 2, test_fwd_add)
  43  (b) group_sum starts at GL / 4 in the W = 8 role: half the group left out
          (test_small_forward 10 and test_small_backward 10: every C whose active lanes fill more than half a group; test_grid_stride_* 8, test_bwd2 6,
          test_bwd_deferred_second_stage 3, test_bwd_ex 2, test_flat_rows 2, test_fwd_add*, 2)
  17  (c) the W = 8 role of ln_bwd_kernel leaves the rows of a group's later trips out of dg
          (test_grid_stride_backward 6: every W = 8 case; test_small_backward 4: C 136, 192, 264, 384, where 33 rows are more than
          one pass; test_bwd2 4, test_bwd_deferred_second_stage 2, test_bwd_ex 1)
   3  (d) the W = 1 role of ln_bwd_kernel keeps gamma for blockIdx.y == 1 (test_bwd2: C 7, 100, 191 -- the three W = 1 cases)
   3  (e) reduce_rows_kernel<8> adds red[r] in the reverse order (test_reduce_rows 9, 63, 64: the bits differ, the bars still hold)
  15  (f) the W = 1 role of ln_fwd_kernel takes lane + 64 j <= C into the variance
          (test_small_forward 10: every W = 1 width but 1; test_scalar_kernels_at_model_widths 96 -- at 192, 384 and 768 no lane has
          lane + 64 j == C, the mutant is the same kernel there; test_flat_rows, test_grid_stride_forward, test_fwd_add* 1 each)
Of these, test_layernorm, test_layernorm_backward_two_gradients_and_scaled_copy and test_layernorm_with_folded_skip_add of
tests/test_gpu_ops.py (fp32 x, aligned, C in 96 / 192 / 200 / 384 / 768, zero-mean rows, whole-tensor rel-L2 at 2e-6 to 1e-4) cannot
see (a) -- on zero-mean data the one-pass rstd is as good as the two-pass one -- nor (d) (no call of csts_layernorm_bwd2), (e) (a
reordering inside 1e-4) and (f) (the W = 1 forms never run); (b) they would see, and (c) at C = 192 and 384, where 210 rows
are several trips.  The mutants were not run against them on the GPU.
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
import layernorm_raw as R                        # noqa: E402
import test_layernorm_reference_host as HOST     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
H = torch.bfloat16
F = torch.float32
PAIRS = [(F, F), (F, H), (H, F), (H, H)]

# Measured bars, about 4x the worst value seen on MI355X against fp64 over every case of this file (the measured value in the
# comment), one constant per storage kind of the tensor the bar is about.
BARS = {
    "rstd_rel": {"f32": 6.4e-7, "bf16": 6.8e-7, "fp16": 6.7e-7},   # by the storage of x, per row: 1.58e-7, 1.70e-7, 1.66e-7
    "k_y": {"f32": 44.0, "bf16": 6.0, "fp16": 6.0},                # K_y by the storage of y: 10.92 (see below), 1.47, 1.53
    "k_dx": {"f32": 12.0, "bf16": 1.2, "fp16": 0.8},               # K_dx by the storage of dx: 2.97, 0.30, 0.19
    "k_dg": {"f32": 12.0, "bf16": 13.0, "fp16": 13.0},             # K_g by the storage of dy: 2.96, 3.15, 3.17
    "k_db": {"f32": 8.0, "bf16": 1.4, "fp16": 2.0},                # K_b by the storage of dy: 1.99, 0.34, 0.48
}
# K_y of fp32 y: 10.92 is one element of `plain` data (rows 33, C 96, row 6, channel 0) where |x_c| + |mean| is 20 times smaller than
# mean_c|x|: S_y prices the error of the mean by |mean|, but it is proportional to mean_c|x|.  The next values are 8.99 and 8.56 (C 767 and
# 383, plain, the same kind of element), then 6.8; a 16-bit y hides such elements under u_out |ref|.  A one-pass variance costs
# K_y >= 214 and an rstd error >= 6.4e-4 on the offset values (tests/test_layernorm_reference_host.py).


def _hold(name, results, half="bf16"):
    """Print the worst figures, then assert every flag and every bar."""
    print(f"\n[{name}] n {len(results)}  " + "  ".join(f"{k} {R.worst(results, k):.3e}" for k in R.DERIVED + R.MEASURED)
          + f"  min var {min((r['min_var'] for r in results if 'min_var' in r), default=float('nan')):.3e}")
    for k in R.MEASURED:                                  # per storage kind, for whoever sets the constants
        for kind in ("f32", "h16"):
            v = [r[k] for r in results if k in r and r["kind"][k] == kind]
            if v:
                print(f"    {k} {kind if kind == 'f32' else half} {max(v):.3e}")
    bad = R.violations(results, BARS, half)
    for r in bad:
        print(f"    MISSED {r}")
    assert not bad, [r["name"] for r in bad]


def test_host_copies_of_the_fp32_bars():
    """tests/test_layernorm_reference_host.py proves on the CPU that the offset values separate a one-pass variance from a two-pass
    one by more than these bars; it cannot import this module where there is no GPU, so it carries copies."""
    assert HOST.RSTD_REL_F32 == BARS["rstd_rel"]["f32"] and HOST.K_Y_F32 == BARS["k_y"]["f32"]


# ------------------------------------------------------------------------------------- every instantiation, small
@pytest.mark.parametrize("C", R.VEC_C + R.SCALAR_C)
def test_small_forward(C):
    _hold(f"small fwd C {C}", R.small_fwd(C, DEV, PAIRS))


@pytest.mark.parametrize("C", R.VEC_C + R.SCALAR_C)
def test_small_backward(C):
    _hold(f"small bwd C {C}", R.small_bwd(C, DEV, PAIRS))


@pytest.mark.parametrize("C", [8, 96, 100, 768])
def test_flat_rows(C):
    """Rows of 3 + 1e-4 randn (variance 1e-8: eps decides rstd) and one exactly constant row, eps 1e-6 and 1e-5."""
    res = []
    for eps in (1e-6, 1e-5):
        for a, b in ((F, F), (H, H)):
            res += R.run_fwd(33, C, a, b, DEV, kind="flat", seed=C, eps=eps) + R.run_bwd(33, C, a, b, DEV, kind="flat", seed=C + 1, eps=eps)
    assert max(r["min_var"] for r in res) < 1e-7
    _hold(f"flat C {C}", res)


# ------------------------------------------------------------------------------------- the W = 1 forms at model widths
@pytest.mark.parametrize("C", R.MISALIGNED_C)
def test_scalar_kernels_at_model_widths(C):
    """One operand at a time off its 16-byte alignment (fp32: one element; 16-bit: one and three): the dispatch must take the
    W = 1 forms of ln_fwd_kernel / ln_bwd_kernel.  Their summation order differs from the W = 8 forms', so only the fp64 bars apply."""
    _hold(f"misaligned C {C}", R.misaligned_cases(DEV, H, C))


# ------------------------------------------------------------------------------------- grid-stride trips
_FWD_TRIPS = R.fwd_trips(H)


@pytest.mark.parametrize("C,rows,xdt,ydt", _FWD_TRIPS, ids=[f"C{c}-rows{r}" for c, r, _, _ in _FWD_TRIPS])
def test_grid_stride_forward(C, rows, xdt, ydt):
    """Rows just past the 4096-workgroup cap of a forward launch: the last rows are a second trip of row0 += ngrp * R."""
    grid, want, per_pass = R.fwd_grid(rows, C, R.is_vec(C))
    assert grid == 4096 < want and per_pass < rows <= 2 * per_pass
    _hold(f"fwd trips C {C} rows {rows}", R.run_fwd(rows, C, xdt, ydt, DEV, kind="offset", seed=C))


_BWD_TRIPS = R.bwd_trips(H)


@pytest.mark.parametrize("C,rows,dydt,xdt,capped", _BWD_TRIPS, ids=[f"C{c}-rows{r}" for c, r, _, _, _ in _BWD_TRIPS])
def test_grid_stride_backward(C, rows, dydt, xdt, capped):
    """Rows past what one pass of a backward launch covers, on offset values, so that the rows of a group's second trip matter to
    dgamma.  The grid is cdiv(rows, 8 waves x rows_per_wave(C)) capped at 512.  At C = 192 and 384 the W = 8 form's lane groups
    take one row per pass and a workgroup holds half as many groups as that formula gives it rows, so every launch of more than 16
    (8) rows takes a second trip, capped or not: 8192 + 19 and 4096 + 9 rows do so on 257 workgroups, 16384 + 19 and 8192 + 9 on
    the capped 512."""
    grid, want, per_pass = R.bwd_grid(rows, C, R.is_vec(C))
    assert grid == R.bwd_partial_rows(rows, C) and (grid == 512 < want) == capped and per_pass < rows
    _hold(f"bwd trips C {C} rows {rows}", R.run_bwd(rows, C, dydt, xdt, DEV, kind="offset", seed=C))


# ------------------------------------------------------------------------------------- csts_layernorm_fwd_add
def test_fwd_add():
    """sum_out is bit-equal to (x.float() + a.float()).to(dtype).  The kernels normalise that sum AS STORED -- for 16-bit x it is
    rounded before the statistics -- so y, mean and rstd are held to the fp64 LayerNorm of the stored sum, which the bit-equality
    ties to the exact one.  (A reference of the unrounded sum is 2^-8 / 2^-11 away from what the kernel computes, by design.)"""
    res = R.fwd_add_cases(DEV, H)
    assert len(res) == 24 and all(r["sum_equal"] is True for r in res)
    _hold("fwd_add", res)


@pytest.mark.parametrize("C", [96, 100])
def test_fwd_add_16bit_sum_consumed_by_backward(C):
    """16-bit x: the backward that follows reads the stored (rounded) sum together with the mean and rstd the forward kernel wrote.
    Held to the fp64 backward of the stored sum with that sum's own statistics.  The regression test of a bug this file found: the
    forward kernels took the statistics of the UNROUNDED fp32 sum, which are not those of the x the backward reads: on MI355X dx
    needed K_dx = 2610 and dgamma K_g = 2918 (bars 1.2 and 13).  They now round a 16-bit sum before the statistics."""
    keep = {}
    res = R.run_fwd(77, C, H, H, DEV, kind="plain", seed=C, add="plain", keep=keep)
    res += R.run_bwd(77, C, H, H, DEV, seed=C + 1, x_data=keep["sum"].float().view(77, C), stats=(keep["mean"], keep["rstd"]))
    _hold(f"fwd_add -> bwd C {C}", res)


# ------------------------------------------------------------------------------------- csts_layernorm_bwd_ex
@pytest.mark.parametrize("C", [96, 100, 384])
def test_bwd_ex(C):
    res = R.bwd_ex_cases(DEV, H, C)
    assert sum("copy_ratio" in r for r in res) == 7 and sum("copy_equal" in r for r in res) == 4 and sum("copy_zero_equal" in r for r in res) == 3
    _hold(f"bwd_ex C {C}", res)


@pytest.mark.parametrize("C,rows", R.DEFERRED)
def test_bwd_deferred_second_stage(C, rows):
    """dgamma == NULL: the call writes the partial rows only; csts_reduce_rows over csts_layernorm_bwd_workspace / (2 C 4) rows
    finishes them (3, 10, 66 and 512 rows: reduce_rows_kernel<2>, <8>, <32>, <32>), bit for bit what the non-deferred call gives."""
    a, b = {}, {}
    res = R.run_bwd(rows, C, H, F, DEV, kind="offset", seed=C, ex=True, keep=a)
    res += R.run_bwd(rows, C, H, F, DEV, kind="offset", seed=C, ex=True, deferred=True, keep=b)
    assert torch.equal(a["dgb"], b["dgb"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["ws"], b["ws"])
    _hold(f"deferred C {C} rows {rows}", res)


# ------------------------------------------------------------------------------------- csts_layernorm_bwd2
@pytest.mark.parametrize("C,rows", R.BWD2, ids=[f"C{c}-rows{r}" for c, r in R.BWD2])
def test_bwd2(C, rows):
    """Two stacked tensors, gamma0 != gamma1, plain values in segment 0 and offset values in segment 1.  C = 7 with 5 rows and
    C = 100 with 77: (rows C) % 8 != 0, and an odd C: the W = 1 form with blockIdx.y == 1.  (With C % 8 == 0 the product is
    always a multiple of 8: that condition can only turn away what C % 8 != 0 has turned away already.)"""
    res = []
    for dydt, xdt in R.bwd2_pairs(C, rows, H):
        res += R.run_bwd2(rows, C, dydt, xdt, DEV, seed=C + rows)
    assert all(r.get("seg0_equal", True) is True for r in res)
    _hold(f"bwd2 C {C} rows {rows}", res)


# ------------------------------------------------------------------------------------- reducers
@pytest.mark.parametrize("nrows", [1, 2, 3, 8, 9, 63, 64, 65, 129, 515])
def test_reduce_rows(nrows):
    """reduce_rows_kernel<2> up to 8 rows, <8> up to 64, <32> above; the 4-way unrolled loop and its remainder; 1 to 48 workgroups
    with a ragged last one."""
    res = []
    for ncols in (1, 31, 32, 33, 192, 1536):
        for scale in (1.0, 0.37):
            res += R.run_reduce(nrows, ncols, scale, DEV)
    _hold(f"reduce_rows {nrows}", res)


def test_reduce_rows_batched():
    """Five descriptors of different widths in one launch of 48 x 5 workgroups: the workgroups past a descriptor's width leave."""
    items = [(1, 1, 1.0), (65, 33, 0.37), (200, 1536, -2.5), (32, 96, 1.0), (129, 31, 0.125)]
    res = R.run_reduce_table(items, 1536, DEV)
    assert sum("single_equal" in r for r in res) == 3
    _hold("reduce_rows_batched", res)


@pytest.mark.parametrize("ncols", [4, 1020, 36864])
def test_reduce_rows_wide(ncols):
    res = R.run_reduce_table([(n, ncols, s) for n, s in ((1, 1.0), (3, 0.37), (4, 1.0), (5, -2.5), (8, 0.37), (13, 1.0))], ncols, DEV, wide=True)
    _hold(f"reduce_rows_wide {ncols}", res)


def test_reduce_rows_wide_two_widths_and_grid_stride():
    """Two descriptors of different widths in one launch (the narrow one's surplus threads find v >= nvec); and 4 (4096 x 256 + 3)
    columns: cdiv(1048579, 256) = 4097 workgroups capped at 4096, the last three float4 columns in a second trip."""
    res = R.run_reduce_table([(3, 1020, 0.37), (5, 36864, 1.0)], 36864, DEV, wide=True)
    ncols = 4 * (4096 * 256 + 3)
    assert -(-(ncols // 4) // 256) == 4097 > 4096
    res += R.run_reduce_table([(2, ncols, 0.37)], ncols, DEV, wide=True)
    _hold("reduce_rows_wide widths / trips", res)


# ------------------------------------------------------------------------------------- fp16
@pytest.fixture(scope="module")
def fp16_child(tmp_path_factory):
    """One child process on libcsts_hip_f16.so, with a timeout."""
    if not os.path.exists(L._PATHS["fp16"]):
        pytest.skip(f"{L._PATHS['fp16']} is not built (make -C csts_amd/csrc f16)")
    path = tmp_path_factory.mktemp("layernorm") / "fp16.json"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSTS_HALF")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "layernorm_worker.py"), str(path)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.load(open(path))


_FP16_CASES = ([f"small_{d}_{C}" for d in ("fwd", "bwd") for C in R.VEC_C + R.SCALAR_C] + ["fwd_add", "bwd_ex_96", "bwd_ex_100", "big", "subnormal"])


@pytest.mark.parametrize("case", _FP16_CASES)
def test_fp16_library(fp16_child, case):
    """libcsts_hip_f16.so: the small table with IEEE-half operands, fwd_add, bwd_ex, |x| near the top of the fp16 range and x in its
    subnormal range (the bars of 16-bit outputs carry + 2^-25)."""
    assert fp16_child["half_kind"] == 1
    res = fp16_child[case]
    assert len(res) >= 12
    _hold(f"fp16 {case}", res, half="fp16")
