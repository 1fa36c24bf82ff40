"""The 3x3x3 depthwise stencil kernels of csts_amd/csrc/stencil.hip, element by element against fp64 (tests/stencil_reference.py),
through raw C-ABI calls on operands inside wider buffers (tests/stencil_raw.py): csts_dwconv_strided, csts_dwconv_transposed /
_transposed2, csts_pool_ln_fwd, csts_dwconv_wgrad / _wgrad2 and csts_dwconv_wgrad_grouped.

Every output region is pre-filled with NaN between sentinel guard bands / foreign slots, every input lives in a buffer that is NaN
outside its own slot: after a call every owned element is finite, nothing else was touched, nothing foreign was read.

Bars (u = 2^-24, u_out = 0 / 2^-8 / 2^-11 for fp32 / bf16 / fp16 outputs):
  convolution outputs (strided, transposed, conv_out)   |err| <= 28 u A (1 + u_out) + u_out |ref|, A = sum |x| |w|     DERIVED
  mean                                                  |err| <= (28 + HD) u mean_head(A)                             DERIVED
  weight gradient                                       |err| <= min(n + 1, C_SWG) u sum |fine| |coarse|              derived / measured
  rstd, y (per (token, head) row, every row)            relative error / row rel-L2 <= RSTD_REL / Y_REL               measured
fp16 outputs add 2^-25 to the convolution bar (half the smallest subnormal: the rounding error of IEEE half below 2^-14).
The derived ratios |err| / bar must be <= 1.  Worst seen on MI355X: convolutions 0.20 (fp32), 0.996 (bf16), 0.999 (fp16) -- with a
16-bit output the bar is the rounding of the output itself, which a value at the bottom of a binade reaches; mean 0.024 (HD 8).
The smallest row variance in any pool_ln_fwd case is 0.020 (HD 8, the one-item case), 0.046 and up elsewhere: no row is near zero.

Mutation check (scratch builds of stencil.hip loaded through CSTS_HIP_LIB, one arithmetic-only change each, no new address and
no longer loop).  Of the 162 tests here, on MI355X, each mutant fails:
  16  dwconv_strided_kernel reads the zero weight row for the valid (kh, kw) = (2, 2) taps when oh == Hc - 1
      (test_ragged_geometries 8, test_strided_dtype_pairs 8)
  20  the 8-channel-per-lane pool_ln_fwd_kernel<16 | 32, 8, ...> leaves its last active lane out of the mean
      (test_pool_ln_head_dims 12, test_grid_cap_pool_ln_generic16 / 32 2 + 2, test_pool_ln_env_variants[cpl0] 4)
   8  dwconv_transposed_s22_kernel drops the (0, 0) tap of its odd-odd output
      (test_transposed_s22_blocks 6, test_ragged_geometries 1, test_grid_cap_s22 1)
  30  dwconv_wgrad_body leaves lane `lanes - 1` out of the LDS fold
      (test_ragged_geometries 18, test_ragged_three_batches_odd_tokens 2, test_wgrad_entries 8, cap / upsample roles 2)
   1  dwconv_strided_kernel stores zeros in its second grid-stride trip (test_grid_cap_strided_and_transposed)
The suite as it stood before cannot see the second mutant (no test set CSTS_POOLLN_CPL12 or pooled with a head_dim other than 96 /
192, so the 8-channel form never ran); the mutants were not run against it on the GPU.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected everywhere, run only on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import lib as L          # noqa: E402
import stencil_raw as R                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
H = torch.bfloat16
F = torch.float32

# Measured bars, about 4x the worst value seen on MI355X against fp64 (the measured value in the comment).
C_SWG = 9.0                                                # weight gradient, units of u sum |fine| |coarse|: 2.29 (fp32), 1.26 (bf16), 1.80 (fp16)
RSTD_REL = {"f32": 9e-7, "h16": 7e-7}                      # rstd per row, relative: 2.2e-7 (fp32, HD 8), 1.8e-7 (16-bit)
Y_REL = {"f32": 1.2e-6, "bf16": 1.3e-2, "fp16": 1.2e-3}    # y per row, rel-L2: 3.0e-7 (fp32), 3.4e-3 (bf16, HD 8), 2.9e-4 (fp16)


def _kind(dt, half="bf16"):
    return "f32" if dt == F else half


def _report(name, conv=(), wgrad=()):
    print(f"\n[{name}] conv ratio {R.worst(conv):.3f}  mean ratio {R.worst(conv, 'mean_ratio'):.3f}  rstd rel {R.worst(conv, 'rstd_rel'):.3e}  "
          f"y rel {R.worst(conv, 'y_rel'):.3e}  min var {min((r['min_var'] for r in conv if 'min_var' in r), default=float('nan')):.3e}  "
          f"wgrad ratio {R.worst(wgrad):.3f}")


def _hold(name, dt, conv=(), wgrad=(), half="bf16"):
    """Print the worst figures, then assert every bar."""
    _report(name, conv, wgrad)
    k = _kind(dt, half)
    bad = R.conv_violations(conv) + R.ln_violations(conv, RSTD_REL["f32" if k == "f32" else "h16"], Y_REL[k]) + R.wgrad_violations(wgrad, C_SWG)
    assert not bad, bad


# ------------------------------------------------------------------------------------- ragged and degenerate geometries
@pytest.mark.parametrize("dt", [F, H], ids=["f32", "bf16"])
@pytest.mark.parametrize("idx", range(len(R.RAGGED)), ids=[f"{f}-{s}".replace(" ", "") for f, s in R.RAGGED])
def test_ragged_geometries(idx, dt):
    """B = 2, C = 192, HD = 96 on odd grids, a last tap outside the grid, the compact (1, 3, 3) stride, extents of one and a stride
    larger than the grid, through strided, transposed, pool_ln_fwd and the weight gradient."""
    conv, wg = R.ragged_all(dt, DEV, idx)
    _hold(f"ragged {R.RAGGED[idx]}", dt, conv, wg)


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "bf16"])
def test_ragged_three_batches_odd_tokens(dt):
    """B = 3 and 27 coarse tokens per batch element: 81 tokens in chunks of 14, so the chunks of the weight gradient cross the
    batch boundaries at 27 and 54 in the middle of a lane's walk."""
    sp = R.Spec(3, 192, 96, (3, 5, 5), (1, 2, 2))
    assert sp.Nc == 27
    conv = R.run_strided(sp, dt, dt, DEV) + R.run_transposed(sp, dt, DEV) + R.run_pool_ln(sp, dt, DEV, nslots=2)
    probs = [R.WgradProblem(sp, dt, DEV)]
    wg = R.run_wgrad(probs, "dweight", DEV) + R.run_wgrad(probs, "null", DEV) + R.run_wgrad_grouped(probs, DEV)
    _hold("B3 odd", dt, conv, wg)


# ------------------------------------------------------------------------------------- every transposed instantiation
_TR_STRIDES = [(a, b, c) for a in (1, 2, 4) for b in (1, 2, 4) for c in (1, 2, 4)] + [(1, 3, 3)]


@pytest.mark.parametrize("st", _TR_STRIDES, ids=["x".join(map(str, s)) for s in _TR_STRIDES])
def test_transposed_every_instantiation(st):
    """dwconv_transposed_kernel<NT, NH, NW>: every axis stride in {1, 2, 4} = 3, 2, 1 candidate taps, in fp32 and bf16, plus the
    non-power-of-two (1, 3, 3).  B = 1, C = 16, HD = 8, fine (5, 7, 6): Hf is odd, so that bf16 does not divert to the 2 x 2-block
    kernel."""
    sp = R.Spec(1, 16, 8, (5, 7, 6), st)
    for dt in (F, H):
        _hold(f"transposed {st}", dt, R.run_transposed(sp, dt, DEV))


@pytest.mark.parametrize("st", [(1, 1, 1), (1, 2, 2), (1, 4, 4)], ids=["333", "322", "311"])
def test_transposed2_two_tables_two_destinations(st):
    """csts_dwconv_transposed2 on the (3,3,3), (3,2,2) and (3,1,1) keys: two weight tables, two sources, two destinations."""
    sp = R.Spec(1, 16, 8, (5, 7, 6), st)
    for dt in (F, H):
        res = R.run_transposed(sp, dt, DEV, nslots=2)
        assert len(res) == 2
        _hold(f"transposed2 {st}", dt, res)


@pytest.mark.parametrize("idx", range(len(R.S22)), ids=[f"{f}-st{s}".replace(" ", "") for f, s in R.S22])
def test_transposed_s22_blocks(idx):
    """dwconv_transposed_s22_kernel<NT>, NT = 3, 2, 1 (st = 1, 2, 4), even grids (3, 8, 12) and (4, 6, 4), one slot and two slots,
    the coarse tensor read in place from a 3C buffer."""
    res = R.s22_all(H, DEV, idx)
    assert len(res) == 3
    _hold(f"s22 {R.S22[idx]}", H, res)


# ------------------------------------------------------------------------------------- strided: dtype pairs
_STRIDED = [((3, 7, 5), (1, 2, 2)), ((4, 14, 14), (1, 8, 8)), ((4, 5, 5), (2, 1, 1)), ((3, 11, 8), (1, 3, 3))]


@pytest.mark.parametrize("pair", [(F, F), (H, H), (F, H), (H, F)], ids=["f32-f32", "bf16-bf16", "f32-bf16", "bf16-f32"])
@pytest.mark.parametrize("fthw,st", _STRIDED, ids=["122", "188", "211", "133"])
def test_strided_dtype_pairs(fthw, st, pair):
    """csts_dwconv_strided called directly, all four (fine, coarse) dtype pairs -- the mixed ones are dwconv_strided_kernel
    <true, false, 4> and <false, true, 4> -- written into a slot of a 3C-wide buffer."""
    sp = R.Spec(2, 192, 96, fthw, st)
    _hold(f"strided {fthw} {st}", pair[1], R.run_strided(sp, pair[0], pair[1], DEV))


# ------------------------------------------------------------------------------------- pool + LayerNorm: head dims
@pytest.mark.parametrize("dt", [F, H], ids=["f32", "bf16"])
@pytest.mark.parametrize("HD", [8, 64, 104, 128, 160, 184, 96, 192])
def test_pool_ln_head_dims(HD, dt):
    """csts_pool_ln_fwd: head dims 8, 64, 104, 128 (8 channels per lane, 16 lanes per item, 1 / 8 / 13 / 16 of them active), 160
    and 184 (32 lanes, 20 / 23 active), 96 and 192 (12 channels per lane, 8 / 16 lanes, all active); heads in {1, 2, 8} while
    C <= 1024, one slot and two slots; conv_out, y, mean and rstd.  Then one workgroup with 1 and with 6 items (R.pool_tiny):
    lane groups that have no item take no part, neither in the shuffles nor in the stores."""
    _hold(f"pool_ln HD {HD}", dt, R.pool_cases(dt, DEV, HD) + R.pool_tiny(dt, DEV, HD))


# ------------------------------------------------------------------------------------- past the grid cap
def test_grid_cap_strided_and_transposed():
    """grid_for_staged caps a launch at 1024 workgroups of 256 threads = 262,144 work items.  B = 2, C = 768, HD = 96, fine
    (2, 27, 27), stride 1: 2 x 1458 tokens x 96 eight-channel chunks = 279,936 items in bf16 (fp32: 192 four-channel chunks,
    559,872): the last 17,792 (297,728) are a second (third) trip through idx += gridDim.x * blockDim.x."""
    sp = R.Spec(2, 768, 96, (2, 27, 27), (1, 1, 1))
    assert sp.B * sp.Nf * (sp.C // 8) == 279936 > 1024 * 256
    _hold("cap strided/transposed bf16", H, R.run_strided(sp, H, H, DEV) + R.run_transposed(sp, H, DEV))
    _hold("cap strided/transposed f32", F, R.run_strided(sp, F, F, DEV, fine_layout="dense", out_layout="dense")
          + R.run_transposed(sp, F, DEV, coarse_layout="dense", out_layout="dense"))


def test_grid_cap_s22():
    """B = 2, C = 768, fine (4, 38, 38), stride (1, 2, 2): 2 x 4 x 19 x 19 blocks x 96 chunks = 277,248 items > 262,144."""
    sp = R.Spec(2, 768, 96, (4, 38, 38), (1, 2, 2))
    assert sp.B * 4 * 19 * 19 * (sp.C // 8) == 277248 > 1024 * 256
    _hold("cap s22", H, R.run_transposed(sp, H, DEV))


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "bf16"])
def test_grid_cap_pool_ln_12_lane(dt):
    """12 channels per lane: 1024 workgroups x 32 items (HD 96: 8 lanes per item) = 32,768.  B = 2, C = 768, HD = 96, fine
    (2, 27, 27), stride 1, two slots: 2 x 1458 x 8 heads x 2 = 46,656 items, the last 13,888 in a second trip of
    item += gridDim.x * groups_per_block."""
    sp = R.Spec(2, 768, 96, (2, 27, 27), (1, 1, 1))
    assert sp.B * sp.Nc * sp.heads * 2 == 46656 > 1024 * 32
    _hold("cap pool12", dt, R.run_pool_ln(sp, dt, DEV, nslots=2, fine_slots=dt != F))      # (fp32: no 3C buffer, to stay small)


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "bf16"])
def test_grid_cap_pool_ln_generic16(dt):
    """8 channels per lane, 16 lanes per item: 1024 x 16 = 16,384 items.  B = 1, C = 192, HD = 64, fine (3, 31, 31), stride 1, two
    slots: 2883 x 3 x 2 = 17,298 items; 17,298 mod 16 = 2: in the workgroup that holds the last two items 14 of 16 groups have
    left the item loop when the other two run their second pass."""
    sp = R.Spec(1, 192, 64, (3, 31, 31), (1, 1, 1))
    assert sp.Nc * sp.heads * 2 == 17298 > 1024 * 16 and 17298 % 16 == 2
    _hold("cap pool16", dt, R.run_pool_ln(sp, dt, DEV, nslots=2))


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "bf16"])
def test_grid_cap_pool_ln_generic32(dt):
    """8 channels per lane, 32 lanes per item: 1024 x 8 = 8,192 items.  B = 1, C = 320, HD = 160, fine (3, 37, 37), one slot:
    4107 x 2 = 8,214 items; 8,214 mod 8 = 6: a ragged second pass."""
    sp = R.Spec(1, 320, 160, (3, 37, 37), (1, 1, 1))
    assert sp.Nc * sp.heads == 8214 > 1024 * 8 and 8214 % 8 == 6
    _hold("cap pool32", dt, R.run_pool_ln(sp, dt, DEV, nslots=1))


# ------------------------------------------------------------------------------------- weight gradients
def _plan(sp):
    """(heads per slab, chunk, chunks, lanes) of csts_dwconv_wgrad, as the host code plans them."""
    k = max(1, 192 // sp.HD)
    while k > 1 and sp.C % (sp.HD * k):
        k -= 1
    nslab, total = sp.C // (sp.HD * k), sp.B * sp.Nc
    nchunk = max(1, min(512 // nslab, -(-total // 16)))
    chunk = -(-total // nchunk)
    return k, chunk, -(-total // chunk), max(1, min(8, 512 // (sp.HD * k // 2), chunk // 2))


def test_wgrad_plan_reaches_the_paths():
    specs = R.wgrad_specs()
    assert [_plan(s)[0] for s in specs[:7]] == [24, 6, 3, 2, 2, 1, 1]
    assert _plan(specs[4])[1:3] == (15, 5) and 72 % 15 != 0
    assert _plan(specs[7])[1:] == (1, 1, 1) and _plan(specs[8])[1:] == (2, 1, 1)
    assert _plan(R.Spec(2, 96, 96, (4, 32, 32), (1, 1, 1)))[2] == 512
    lib = L.load()
    for s in specs:       # the workspace the library asks for is the one this plan implies
        p = R.WgradProblem(s, H, DEV)
        assert lib.csts_dwconv_wgrad_workspace(C.byref(p.g)) == _plan(s)[2] * (s.C // (s.HD * _plan(s)[0])) * s.HD * 27 * 4


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["dweight", "null", "two", "grouped"])
def test_wgrad_entries(mode, dt):
    """csts_dwconv_wgrad with dweight given (second stage inside the call) and NULL (partial rows summed here), csts_dwconv_wgrad2
    (two problems per launch, dweight given for one, NULL for the other) and the grouped launch, on the same problems."""
    specs = R.wgrad_specs()
    if mode == "two":
        res = R.run_wgrad([(R.WgradProblem(s, dt, DEV, seed=4), R.WgradProblem(s, dt, DEV, seed=14)) for s in specs], "two", DEV)
        assert len(res) == 2 * len(specs)
    elif mode == "grouped":
        res = R.run_wgrad_grouped([R.WgradProblem(s, dt, DEV) for s in specs], DEV)
    else:
        res = R.run_wgrad([R.WgradProblem(s, dt, DEV) for s in specs], mode, DEV)
    _hold(f"wgrad {mode}", dt, wgrad=res)


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "bf16"])
def test_wgrad_workgroup_cap_and_upsample_roles(dt):
    """B = 2, C = 96, coarse 4 x 32 x 32: 8192 tokens = 512 chunks of 16, the cap of the plan; and the decoder's roles (fine = the
    dense gradient, coarse = a slot of the qkv buffer) on a (2, 1, 1) and a (1, 2, 2) upsampling, single and grouped."""
    cap = R.WgradProblem(R.Spec(2, 96, 96, (4, 32, 32), (1, 1, 1)), dt, DEV)
    ups = [R.WgradProblem(R.Spec(2, 192, 96, (4, 5, 5), (2, 1, 1)), dt, DEV, roles="upsample"),
           R.WgradProblem(R.Spec(2, 192, 96, (3, 8, 12), (1, 2, 2)), dt, DEV, roles="upsample")]
    res = R.run_wgrad([cap] + ups, "dweight", DEV) + R.run_wgrad([cap] + ups, "null", DEV) + R.run_wgrad_grouped([cap] + ups, DEV)
    _hold("wgrad cap / upsample roles", dt, wgrad=res)


# ------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    """Host checks: each of these calls returns non-zero and leaves every output as it was."""
    lib = L.load()
    s = R.stream()
    sp = R.Spec(1, 16, 8, (2, 4, 4), (1, 2, 2))
    fine = sp.fine_region(H, DEV, ("slot", 1)).load(R.rand((1, sp.Nf, 16), 1, DEV))
    coarse = sp.coarse_region(H, DEV, ("rows", 8)).load(R.rand((1, sp.Nc, 16), 2, DEV))
    fine32 = sp.fine_region(F, DEV, ("slot", 1)).load(R.rand((1, sp.Nf, 16), 1, DEV))
    out_c, out_f = sp.coarse_region(H, DEV, ("rows", 8)).arm(), sp.fine_region(H, DEV, ("slot", 1)).arm()
    y = sp.coarse_region(H, DEV, ("rows", 8)).arm()
    rows = sp.Nc * sp.heads
    mean, rstd = R._f32_out(rows, DEV), R._f32_out(rows, DEV)
    w = R.weights(8, 3, DEV)
    gamma, beta = R.ln_params(8, 4, DEV)
    good = sp.geom(fine, coarse)
    wsz = lib.csts_dwconv_wgrad_workspace(C.byref(good))
    ws, dw = R._f32_out(wsz // 4, DEV), R._f32_out(8 * 27, DEV)

    def geom(**kw):
        g = sp.geom(fine, coarse)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def strided(g, fp=fine.ptr(), op=None):
        return lib.csts_dwconv_strided(C.byref(g), fp, L.BF16, w.data_ptr(), out_c.ptr() if op is None else op, L.BF16, s)

    def transposed(g, cp=coarse.ptr(), cdt=L.BF16, op=None):
        return lib.csts_dwconv_transposed(C.byref(g), cp, cdt, w.data_ptr(), out_f.ptr() if op is None else op, L.BF16, s)

    def wgrad(g, fdt=L.BF16, fp=fine.ptr(), nbytes=wsz):
        return lib.csts_dwconv_wgrad(C.byref(g), fp, fdt, coarse.ptr(), L.BF16, dw.ptr(), ws.ptr(), nbytes, s)

    def pool(g, nslots=1, fp=fine.ptr(), cp=None):
        pa = L.PoolLnArgs()
        pa.geom, pa.nslots, pa.dt, pa.eps = g, nslots, L.BF16, 1e-5
        for i in range(min(nslots, 2)):
            pa.fine[i], pa.weight[i], pa.gamma[i], pa.beta[i] = fp, w.data_ptr(), gamma.data_ptr(), beta.data_ptr()
            pa.conv_out[i], pa.y[i], pa.mean[i], pa.rstd[i] = out_c.ptr() if cp is None else cp, y.ptr(), mean.ptr(), rstd.ptr()
        return lib.csts_pool_ln_fwd(C.byref(pa), s)

    bad_geoms = {
        "HD % 8": geom(C=12, HD=12), "stride 0": geom(sh=0), "coarse grid": geom(Hc=sp.cthw[1] + 1),
        "token stride % 8": geom(fine_token_stride=fine.ts + 4), "coarse token stride % 8": geom(coarse_token_stride=coarse.ts + 4),
    }
    for name, g in bad_geoms.items():
        assert strided(g) != 0 and transposed(g) != 0 and wgrad(g) != 0 and pool(g) != 0, name
    assert strided(good, fp=fine.ptr() + 8) != 0 and strided(good, op=out_c.ptr() + 8) != 0, "misaligned base"
    assert transposed(good, cp=coarse.ptr() + 8) != 0 and transposed(good, op=out_f.ptr() + 8) != 0, "misaligned base"
    assert pool(good, fp=fine.ptr() + 8) != 0 and pool(good, cp=out_c.ptr() + 8) != 0, "misaligned base"
    g32 = sp.geom(fine32, coarse)
    assert transposed(good, cdt=L.F32) != 0, "transposed: mixed dtypes"
    assert wgrad(g32, fdt=L.F32, fp=fine32.ptr()) != 0, "wgrad: mixed dtypes"
    assert pool(good, nslots=3) != 0 and pool(good, nslots=0) != 0, "nslots"
    assert wgrad(good, nbytes=wsz - 1) != 0, "workspace one byte short"
    torch.cuda.synchronize()
    for o in (out_c, out_f, y, mean, rstd, ws, dw):           # nothing was launched: prefill and sentinel as armed
        assert o.guards_ok() and bool((o.ibuf[o.mask] == R._sx(R.PREFILL[o.es], o.es)).all())
    # and the same operands are accepted once the argument is right
    assert strided(good) == 0 and transposed(good) == 0 and wgrad(good) == 0 and pool(good) == 0
    torch.cuda.synchronize()
    assert out_c.finite() and out_f.finite() and dw.finite() and y.finite()


# ------------------------------------------------------------------------------------- environment variants and fp16
_CHILDREN = [("cpl0", {"CSTS_POOLLN_CPL12": "0"}), ("cpl2", {"CSTS_POOLLN_CPL12": "2"}), ("fp16", {})]


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """Three child processes, one after another, each with a timeout; the first that dies ends the run (no further child starts)."""
    out = {}
    d = tmp_path_factory.mktemp("stencil")
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSTS_HALF", "CSTS_POOLLN_CPL12")}
    for mode, extra in _CHILDREN:
        path = d / f"{mode}.json"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stencil_worker.py"), mode, str(path)], cwd=ROOT,
                           env={**base, **extra}, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (mode, p.stderr[-4000:])
        out[mode] = json.load(open(path))
    return out


@pytest.mark.parametrize("mode", ["cpl0", "cpl2"])
@pytest.mark.parametrize("case", [f"pool_hd{hd}_{t}" for hd in (96, 192) for t in ("f32", "h16")])
def test_pool_ln_env_variants(children, mode, case):
    """CSTS_POOLLN_CPL12=0: head dims 96 and 192 on 8 channels per lane (12 of 16 and 24 of 32 lanes active);
    CSTS_POOLLN_CPL12=2: the ALL27 form of the 12-channel kernel for 16-bit operands.  The pool_cases of test_pool_ln_head_dims, same bars."""
    r = children[mode]
    assert r["half_kind"] == 0 and r["cpl12"] == mode[3]
    assert len(r[case]["conv"]) == (9 if "hd96" in case else 6)       # 3 / 2 head counts x (1 + 2) slots
    _hold(f"{mode} {case}", F if case.endswith("f32") else H, r[case]["conv"])


@pytest.mark.parametrize("sfx", ["", "_big", "_subnormal"], ids=["ordinary", "big", "subnormal"])
@pytest.mark.parametrize("case", [f"ragged{i}" for i in range(len(R.RAGGED))] + [f"s22_{i}" for i in range(len(R.S22))])
def test_fp16_library(children, case, sfx):
    """libcsts_hip_f16.so: the ragged table through all four kernels and the 2 x 2-block transposed cases with IEEE-half operands --
    ordinary values, values near the top of the fp16 range, channels in its subnormal range (bar + 2^-25 for fp16 outputs)."""
    r = children["fp16"]
    assert r["half_kind"] == 1
    res = r[case + sfx]
    assert len(res["conv"]) == 3 and len(res["wgrad"]) == (0 if case.startswith("s22") else 1)
    _hold(f"fp16 {case}{sfx}", torch.float16, res["conv"], res["wgrad"], half="fp16")
