"""Host checks of the GEMM pin (tests/gemm_reference.py, tests/gemm_raw.py, tests/test_gpu_gemm.py); no GPU.

Coverage.  Every case of gemm_raw's tables is put to csts_gemm_kernel_name with made-up aligned pointers (host-only, as
tools/gemm_route_table.py does) in a child process whose CSTS_GEMM* variables are removed.  The name must be the one the table
expects, and the set of names must equal gemm_raw.expected_instantiations(): every instantiation csts_gemm, launch4 and launch5 can
start -- 6 gemm_kernel, 6 gemm_tiny_kernel, 21 gemm2_kernel (a forced 256 rows with fp32 A falls back to the automatic tile), 8
gemm3_kernel, every G4_VARIANTS code x every form it instantiates (6 x 1 + 11 x 6 = 72), 22 gemm5_kernel -- each at least once on
`exact` values and once on random ones.  The split-K finishing pass has no name query: the (VEC, SL) launch_finish_v would choose
is mirrored from the shapes (gemm_reference.finish_form) and all six must occur.

Sensitivity.  For each case the fp64 reference is compared with fp64 emulations of wrong kernels (gemm_reference.MUTANTS): the last
16 of K left out, the last split slab left out, the bias of column n ^ 1, the residual added before the row scale, the scale of row
m - 1, row m instead of m % res_row_mod, tanh-GELU instead of erf-GELU (fp32 C).  The worst |difference| / bar over the case's
elements must be >= 4 wherever the mutant applies.  The bar is the derived one, lowered to the measured constant where C is fp32:
K_F32 and CF below are copies of tests/test_gpu_gemm.py's BARS (that module asserts they are equal; it cannot be imported here).

Self-checks of the reference: NT / NN / TN agree on transposed inputs, `exact` sets satisfy the 2^24 condition (reference() asserts
it), the res_up reference equals F.interpolate(mode="trilinear") in fp64, the erf-GELU equals torch's."""
import json
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import gemm_reference as GR        # noqa: E402
import gemm_raw as R               # noqa: E402

H = torch.bfloat16
# copies of BARS["k"][family]["f32"] and BARS["cf"] of tests/test_gpu_gemm.py
K_F32 = {"gemm_tiny": 10.3, "gemm": 28.2, "gemm2": 20.3, "gemm3": 27.3, "gemm4": 29.8, "gemm5": 26.3}
CF = {"gelu_fast": 1.0, "dgelu_fast": 2.3, "gelu_libm": 5.6, "dgelu_libm": 3.1}
FACTOR = 4.0


def _child(out_path):
    names = {cid: R.host_name(c) for cid, _, c in R.all_cases() + R.fp16_cases() + R.switch_cases()}
    with open(out_path, "w") as f:
        json.dump(names, f)


@pytest.fixture(scope="module")
def names(tmp_path_factory):
    """case id -> (kernel name, k-splits), asked in a child process without the library's CSTS_GEMM* switches."""
    out = tmp_path_factory.mktemp("gemm") / "names.json"
    env = {k: v for k, v in os.environ.items() if not k.startswith("CSTS_GEMM")}
    env["CSTS_HALF"] = "bf16"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.load(open(out))


def test_case_ids_are_unique():
    ids = [cid for cid, _, _ in R.all_cases()]
    assert len(ids) == len(set(ids))


def test_every_case_routes_to_the_kernel_it_names(names):
    bad = [(cid, want, names[cid][0]) for cid, want, _ in R.all_cases() + R.fp16_cases() if names[cid][0] != want]
    assert not bad, (len(bad), bad[:5])
    # under algo 0 and without the switches, the switch-reached kernels are NOT what these problems take
    assert all(names[cid][0] != want for cid, want, _ in R.switch_cases() if "res-lines" not in cid)


def test_every_instantiation_is_covered_on_exact_and_on_random_values(names):
    want = R.expected_instantiations()
    assert len(want) == 6 + 6 + 21 + 8 + 72 + 22 and len(set(want)) == len(want)
    by_kind = {True: set(), False: set()}
    for cid, _, c in R.all_cases():
        by_kind[c["kind"] == "exact"].add(names[cid][0])
    assert sorted(by_kind[True] | by_kind[False]) == want, (sorted(set(want) - by_kind[True] - by_kind[False]),
                                                             sorted((by_kind[True] | by_kind[False]) - set(want)))
    # (the finishing-pass cases run on random values only: their check is the exact-order emulation)
    assert by_kind[True] == set(want) and by_kind[False] == set(want), sorted(set(want) - by_kind[True]) + sorted(set(want) - by_kind[False])


def test_every_finishing_form_is_covered(names):
    forms = set()
    for cid, _, c in R.all_cases():
        if c["split"] > 1 and c["det"]:
            k_chunk, nsplit = GR.split_plan(c, names[cid][0])
            assert nsplit == names[cid][1], cid
            forms.add(GR.finish_form(c, nsplit))
    assert sorted(forms) == R.FINISH_FORMS
    assert sorted(GR.finish_form(c, GR.split_plan(c, n)[1]) for _, n, c in R.finish_cases()[:6]) == R.FINISH_FORMS


def test_split_k_at_k_40_gives_fewer_slabs_than_asked_for(names):
    hit = [(cid, names[cid][1]) for cid, _, c in R.all_cases() if c["split"] == 3 and c["K"] == 40]
    assert hit and all(n == 2 for _, n in hit), hit
    assert all(names[cid][1] == 3 for cid, _, c in R.all_cases() if c["split"] == 3 and c["K"] == 200)


# ------------------------------------------------------------------------------------------------------------ sensitivity
def _k(c, r, name):
    fam = name.split("_kernel")[0]
    return min(r["c_derived"], K_F32[fam]) if c["c"] == "f32" else r["c_derived"]


@pytest.mark.parametrize("table", list(R.TABLES))
def test_wrong_kernels_miss_the_bars(names, table):
    """Each mutant, on every case it applies to, is at least FACTOR bars away from the reference at its worst element."""
    weak, seen = [], {m: 0 for m in GR.MUTANTS}
    for cid, _, c in R.TABLES[table]():
        name = names[cid][0]
        plan = GR.split_plan(c, name) if c["split"] > 1 else (c["K"], 1)
        todo = [m for m in GR.MUTANTS if GR.applies(m, c, plan)]
        if not todo:
            continue
        o = GR.operands(c, H)
        fn = GR.fn_kind(c, name)
        r = GR.reference(c, o, H, fn, plan)
        fn_key = f"{c['epi']}_{fn}"
        bar = GR.bar(r, _k(c, r, name), CF.get(fn_key, 0.0), GR.dt(c["c"], H))
        for m in todo:
            d = (GR.reference(c, o, H, fn, plan, mutant=m)["C64"] - r["C64"]).abs()
            ratio = R._worst(d, bar)[0]
            seen[m] += 1
            if not ratio >= FACTOR:
                weak.append((cid, m, ratio))
    print(f"\n[{table}] cases per mutant: {seen}")
    assert not weak, (len(weak), weak[:40])


def test_every_mutant_meets_some_case(names):
    seen = set()
    for cid, _, c in R.all_cases():
        plan = GR.split_plan(c, names[cid][0]) if c["split"] > 1 else (c["K"], 1)
        seen |= {m for m in GR.MUTANTS if GR.applies(m, c, plan)}
    assert seen == set(GR.MUTANTS)


# ------------------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("kind", ["plain", "exact"])
def test_layouts_agree_on_transposed_inputs(kind):
    kw = dict(bias=True, epi="gelu", aux="f32", rps=10, res="f32", res_row_mod=20, c="f32", kind=kind, seed=3)
    c = {l: GR.case(l, 65, 97, 40, **kw) for l in ("NT", "NN", "TN")}
    o = GR.operands(c["NT"], H)
    r = {"NT": GR.reference(c["NT"], o, H, "libm")}
    r["NN"] = GR.reference(c["NN"], dict(o, B=o["B"].t().contiguous()), H, "libm")
    r["TN"] = GR.reference(c["TN"], dict(o, A=o["A"].t().contiguous(), B=o["B"].t().contiguous()), H, "libm")
    for l in ("NN", "TN"):
        for key in ("C64", "pre64", "S", "S_pre"):
            assert torch.equal(r[l][key], r["NT"][key]), (l, key)
    # and the reference is the plain formula
    a, b = o["A"].double(), o["B"].double()
    pre = a @ b.t() + o["bias"].double()
    want = torch.nn.functional.gelu(pre) * o["row_scale"].double()[torch.arange(65) // 10].view(65, 1) + o["residual"].double()[torch.arange(65) % 20]
    assert torch.allclose(r["NT"]["C64"], want, rtol=1e-13, atol=1e-13)


def test_operands_are_rounded_as_the_mfma_reads_them():
    c = GR.case("NN", 9, 8, 16, a="f32", b="f32", c="f32")
    o = GR.operands(c, H)
    assert o["A"].dtype == torch.float32 and not torch.equal(o["A"], o["A"].to(H).float())
    r16 = GR.reference(c, o, H)
    assert torch.equal(r16["C64"], o["A"].to(H).double() @ o["B"].to(H).double())
    r32 = GR.reference(dict(c, compute="f32"), o, H)
    assert torch.equal(r32["C64"], o["A"].double() @ o["B"].double())


def test_exact_sets_are_exact_in_fp32():
    """Integers below 2^24 whatever the order: the fp32 matmul of torch, in its own order, gives the fp64 result bit for bit."""
    for cid, _, c in R.all_cases():
        if c["kind"] != "exact" or c["M"] * c["N"] > 1 << 16:
            continue
        o = GR.operands(c, H)
        r = GR.reference(c, o, H)               # asserts the 2^24 condition
        if c["epi"] == "none" and c["res"] is None and c["rps"] == 0:
            A, B = o["A"].float(), o["B"].float()
            p32 = (A.t() if c["layout"] == "TN" else A) @ (B.t() if c["layout"] == "NT" else B)
            if o["bias"] is not None:
                p32 = p32 + o["bias"]
            assert torch.equal(p32.double(), r["C64"]), cid


def test_res_up_is_trilinear_interpolation():
    g = torch.Generator().manual_seed(5)
    for grids in (R.UP, (3, 2, 5, 4, 8, 8), (1, 1, 1, 2, 2, 4)):
        Ti, Hi, Wi, To, Ho, Wo = grids
        r = torch.randn(2 * Ti * Hi * Wi, 7, generator=g, dtype=torch.float64)
        got, ab = GR.res_up64(r, grids, 2 * To * Ho * Wo)
        want = torch.nn.functional.interpolate(r.view(2, Ti, Hi, Wi, 7).permute(0, 4, 1, 2, 3), size=(To, Ho, Wo), mode="trilinear",
                                               align_corners=False).permute(0, 2, 3, 4, 1).reshape(-1, 7)
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13) and bool((ab >= got.abs() - 1e-12).all())
    assert GR.dyadic_up(R.UP) and not GR.dyadic_up((3, 2, 5, 4, 8, 8))


def test_gelu_functions():
    x = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    assert torch.allclose(GR.gelu64(x), torch.nn.functional.gelu(x), rtol=0, atol=1e-15)
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(xr).sum().backward()
    assert torch.allclose(GR.dgelu64(x), xr.grad, rtol=0, atol=1e-14)
    assert torch.allclose(GR.gelu_tanh64(x), torch.nn.functional.gelu(x, approximate="tanh"), rtol=0, atol=1e-14)


def test_finish_emulation_is_a_sum_in_lane_order():
    ws = GR.operands(GR.case("NT", 17, 4, 16, **R.F32C), H)["A"].view(17, 4, 4)
    for SL in (1, 4, 16):
        v = GR.finish_emulation(ws, 17, SL, None, torch.float32)
        assert torch.allclose(v.double(), ws.double().sum(0), rtol=1e-6, atol=1e-6)
    assert not torch.equal(GR.finish_emulation(ws, 17, 1, None, torch.float32), GR.finish_emulation(ws, 17, 16, None, torch.float32))


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
