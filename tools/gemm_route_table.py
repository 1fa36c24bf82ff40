"""The routing table of csts_gemm: for a fixed list of problems, which kernel the library names (csts_gemm_kernel_name), with how
many k-splits, and what csts_gemm_plan answers.  Both queries are host-only, so this runs without a GPU; the operand pointers
are made-up 256-byte-aligned integers that nothing dereferences.

    python tools/gemm_route_table.py [--lib path/to/libcsts_hip.so] [--out file]

One line per case:  <case> | <kernel name, or "rc -1" and the csts_last_error message> | <k-splits> | <v2 tile_rows nsplit of the plan, or "rc -1">

The table is printed by a child process whose environment has every CSTS_GEMM* variable removed (the library reads its A/B
switches once per process).  tests/test_gemm_route_host.py compares the output with tests/golden/gemm_routes.txt; gemm_args()
and kernel_name() below are also what a test uses to ask for one name."""
import argparse
import ctypes as C
import itertools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from csts_amd import lib as L   # noqa: E402

DT = {"f32": L.F32, "bf16": L.BF16}
LAYOUT = {"NT": L.GEMM_NT, "NN": L.GEMM_NN, "TN": L.GEMM_TN}
EPI = {"none": L.EPI_NONE, "gelu": L.EPI_GELU, "dgelu": L.EPI_DGELU}
# made-up operand addresses, 256-byte aligned, 4 GiB apart
FAKE = {n: (i + 1) << 32 for i, n in enumerate(("A", "B", "C", "bias", "aux", "residual", "row_scale", "workspace", "colsum"))}


def gemm_args(layout, M, N, K, *, a="bf16", b="bf16", c="bf16", compute="bf16", epi="none", bias=False, aux=None, res=None,
              res_row_mod=0, rps=0, split=1, ws=False, colsum=False, tile_rows=0, algo=0, res_up=None, ld_pad=0, ptr_off=0,
              ptrs=None):
    """A csts_gemm_args for the problem.  aux / res: dtype name of the operand, or None for absent; rps > 0: a row scale for every
    rps rows; ws: a split-k workspace of the size csts_gemm_splitk_workspace asks for; ld_pad / ptr_off: elements added to every
    leading dimension / bytes added to the A pointer (misaligned operands); ptrs: real addresses by operand name (default: FAKE)."""
    p = dict(FAKE, **(ptrs or {}))
    g = L.GemmArgs()
    g.layout = LAYOUT[layout]
    g.M, g.N, g.K = M, N, K
    g.A, g.a_dt, g.lda = p["A"] + ptr_off, DT[a], (M if layout == "TN" else K) + ld_pad
    g.B, g.b_dt, g.ldb = p["B"], DT[b], (K if layout == "NT" else N) + ld_pad
    g.C, g.c_dt, g.ldc = p["C"], DT[c], N + ld_pad
    g.bias = p["bias"] if bias else None
    g.epilogue = EPI[epi]
    if aux is not None:
        g.aux, g.aux_dt, g.ldaux = p["aux"], DT[aux], N + ld_pad
    elif epi == "gelu":
        g.aux_dt = DT[c]             # the GELU flavour follows the activation dtype when the pre-activation is not kept
    if res is not None:
        g.residual, g.r_dt, g.ldr, g.res_row_mod = p["residual"], DT[res], N + ld_pad, res_row_mod
    if rps > 0:
        g.row_scale, g.rows_per_scale = p["row_scale"], rps
    g.compute, g.split_k, g.tile_rows, g.algo = DT[compute], split, tile_rows, algo
    if ws:
        g.workspace, g.ws_bytes = p["workspace"], L.load().csts_gemm_splitk_workspace(M, N, K, split)
    if colsum:
        g.colsum = p["colsum"]
    for i, v in enumerate(res_up or ()):
        g.res_up[i] = v
    return g


def kernel_name(g):
    """(return code, kernel name as rocprofv3 prints it -- or the error message --, k-splits) of csts_gemm_kernel_name."""
    lib = L.load()
    buf, ns = C.create_string_buffer(160), C.c_int(0)
    rc = lib.csts_gemm_kernel_name(C.byref(g), buf, 160, C.byref(ns))
    return rc, (buf.value.decode() if rc == 0 else (lib.csts_last_error() or b"").decode()), ns.value


def plan(g):
    v2, rows, ns = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = L.load().csts_gemm_plan(C.byref(g), C.byref(v2), C.byref(rows), C.byref(ns))
    return rc, v2.value, rows.value, ns.value


# ------------------------------------------------------------------------------------------------ the cases
F32C = dict(a="f32", b="f32", c="f32", compute="f32")
RES = dict(c="f32", bias=True, res="f32")                            # proj / fc2 onto the fp32 residual stream
GELU = dict(bias=True, epi="gelu", aux="bf16")                       # fc1, pre-activation kept
# epilogue forms of the train step, as keyword sets of gemm_args
STEP_FORMS = {
    "NT": [dict(), GELU, dict(epi="dgelu", aux="bf16"), RES, dict(c="f32", bias=True)],
    "NN": [dict(a="f32", c="f32"), dict()],
    "TN": [dict(a="f32", c="f32"), dict(c="f32"), dict(a="f32", c="f32", colsum=True)],
}
# the GEMM tests of tests/test_gpu_ops.py: shapes run in all three layouts and both compute types, and NT-only shapes with the
# epilogues those tests use
LAYOUT_SHAPES = [(300, 200, 96), (1040, 768, 264), (128, 128, 32), (16, 768, 4096), (65, 97, 40), (520, 384, 96)]
NT_SHAPES = [(520, 384, 96), (2080, 160, 448), (777, 288, 160), (4096, 1536, 384), (300, 96, 1040), (33000, 192, 64), (2048, 384, 192),
             (1024, 96, 192), (2048, 768, 768), (16384, 96, 96), (16416, 384, 96), (16384, 192, 96), (19968, 96, 192), (16384, 288, 192),
             (16384, 768, 96), (16608, 96, 384), (16384, 288, 384)]
NT_TEST_FORMS = [dict(), dict(bias=True), GELU, dict(bias=True, epi="gelu"), dict(epi="dgelu", aux="bf16"), dict(c="f32", epi="dgelu", aux="bf16"),
                 dict(c="f32", bias=True), RES, dict(RES, rps=100), dict(RES, res_row_mod=-2, rps=-2)]
# every forced algo the tests and tools/gemm4_lab.py use, and codes that do not exist
ALGOS = [2, 312, 313, 314, 322, 323, 324, 1322, 342, 343, 402, 403, 412, 422, 432, 433, 434, 442, 452, 462, 463, 472, 473, 474, 483, 484,
         500, 503, 506, 311, 344, 499]
# problems the forced kernels apply to, and ones they do not (K % 8, K % 64, N % 96 and M % 32, split-k, layout)
ALGO_SHAPES = [("NT", 8192, 1536, 384, 1), ("NT", 8192, 384, 1536, 1), ("NT", 16384, 192, 192, 1), ("NT", 8192, 384, 100, 1),
               ("NT", 8192, 384, 720, 1), ("NT", 1000, 100, 384, 1), ("NT", 8192, 384, 1536, 2), ("TN", 768, 3072, 8192, 1)]


def file_shapes():
    """(layout, M, N, K, split) of the replayed train step and of the M = 8192 / 2048 lab shapes, in file order, each once."""
    seen, out = set(), []
    for line in open(os.path.join(ROOT, "profiles", "r5_final_gemm_replay_shapes.txt")):
        f = line.split()
        if len(f) > 5 and f[0] in LAYOUT:
            out.append((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])))
    for line in open(os.path.join(ROOT, "tools", "shapes_m8192.txt")):
        f = line.split()
        if len(f) >= 3 and not line.startswith("#"):
            out.append(("NT", int(f[0]), int(f[1]), int(f[2]), 1))
    return [s for s in out if not (s in seen or seen.add(s))]


def case_label(layout, M, N, K, **kw):
    """The first column of a case's line: the problem and every gemm_args keyword that is set."""
    return (f"{layout} {M} {N} {K} " + " ".join(k if v is True else f"{k}={v}" for k, v in sorted(kw.items())
                                                if v not in (None, False, 0) and (k, v) != ("split", 1))).rstrip()


def cases():
    """(label, csts_gemm_args) of every case, in a fixed order."""
    out, seen = [], set()

    def add(layout, M, N, K, **kw):
        for k in ("res_row_mod", "rps"):
            if kw.get(k) == -2:
                kw[k] = (M + 1) // 2
        if kw.get("split", 1) <= 1:
            kw.pop("ws", None)
        label = case_label(layout, M, N, K, **kw)
        if label not in seen:
            seen.add(label)
            out.append((label, gemm_args(layout, M, N, K, **kw)))

    # 1. the shapes of the step under the epilogue forms of their layout, the shapes and epilogues of the tests
    for layout, M, N, K, split in file_shapes():
        for form in STEP_FORMS[layout]:
            add(layout, M, N, K, split=split, ws=True, **form)
    for (M, N, K), layout in itertools.product(LAYOUT_SHAPES, LAYOUT):
        add(layout, M, N, K, b="f32", c="f32")
        add(layout, M, N, K, **F32C)
        add(layout, M, N, K, split=3, **F32C)                                  # split-k with atomics
        add(layout, M, N, K, b="f32", c="f32", split=3, ws=True)
    for (M, N, K), form in itertools.product(NT_SHAPES, NT_TEST_FORMS):
        add("NT", M, N, K, **form)
    # 2. either side of the heuristic edges, bf16 and fp32 residual-stream outputs.  Rows: pick3 256, pick4 2048, pick5 16384
    for (M, N, K), form in itertools.product(((255, 384, 1536), (256, 384, 1536), (2047, 768, 768), (2048, 768, 768), (16383, 384, 192),
                                              (16352, 384, 192), (16384, 384, 192), (16384, 384, 384)), (GELU, RES)):
        add("NT", M, N, K, **form)
    # tiles of 128 x 192 (pick4: 128, 256; with K >= 1536 the 3-stage ring at exactly 256) and of 128 x 128 (pick4: 128 .. 512; pick3 and
    # pick_tile_rows: 512), one row tile less and the edge itself
    for (rows, N), K, form in itertools.product(((127, 192), (128, 192), (255, 192), (256, 192), (257, 192), (127, 128), (128, 128), (511, 128),
                                                 (512, 128), (513, 128), (63, 384), (64, 384)), (768, 1536), (GELU, RES)):
        add("NT", 128 * rows, N, K, **form)
    # K: pick3 768, pick4 1024 / 1536 and K % 64, v3_ok K % 16, v2_ok K % 8; N % 192, N % 128, N % 96 only, none
    for (N, K), form in itertools.product(((384, 704), (384, 720), (384, 760), (384, 767), (384, 768), (256, 960), (256, 1024), (1536, 1472),
                                           (1536, 1536), (192, 768), (128, 768), (288, 768), (160, 768)), (GELU, RES)):
        add("NT", 1024, N, K, **form)
        add("NT", 8192, N, K, **form)
    # tiny_ok: K <= 16 with up to 2^20 outputs, or up to 8192 outputs with K <= 8192; plain fp32 with at most a bias
    for layout, (M, N, K) in itertools.product(LAYOUT, ((1024, 1024, 16), (1025, 1024, 16), (1024, 1024, 17), (64, 128, 17), (65, 128, 17),
                                                        (64, 128, 8192), (64, 128, 8193), (4, 256, 4), (4, 768, 256))):
        add(layout, M, N, K, **F32C)
    for form in (dict(bias=True), dict(epi="gelu"), dict(compute="bf16"), dict(split=2)):
        add("NT", 4, 256, 4, **dict(F32C, **form))
    # pick_tile_rows: weight gradients (256 rows where that pads no further and fills the chip), forced tiles
    for M, N, split in itertools.product((96, 128, 256, 384, 768), (768, 3072), (1, 8, 64)):
        add("TN", M, N, 8192, a="f32", c="f32", split=split, ws=True)
        add("TN", M, N, 8192, c="f32", split=split, ws=True, colsum=True)
    for layout, (M, N, K), tile in itertools.product(LAYOUT, ((8192, 1536, 384), (100, 384, 768)), (64, 128, 256, 32)):
        add(layout, M, N, K, c="f32", tile_rows=tile)
        add(layout, M, N, K, a="f32", c="f32", tile_rows=tile)
    # 3. operands the vector kernels cannot take: odd leading dimensions, a pointer off by two bytes
    for layout, (M, N, K) in itertools.product(LAYOUT, ((8192, 1536, 384), (16384, 192, 192))):
        for form in (dict(), RES, dict(c="f32", colsum=True)):
            if "colsum" not in form or layout == "TN":
                add(layout, M, N, K, ld_pad=1, **form)
                add(layout, M, N, K, ld_pad=4, **form)
                add(layout, M, N, K, ptr_off=2, **form)
    # 4. the up-sampled residual of the decoder (M = B * To * Ho * Wo)
    for algo, (N, K) in itertools.product((0, 2, 313, 463, 500), ((768, 768), (384, 768), (192, 192))):
        add("NT", 8192, N, K, res_up=(4, 16, 16, 8, 32, 32), algo=algo, **RES)
    # 5. forced kernels, each on problems it applies to and on ones it does not; the 16-bit and the repeating residual on one of them
    for algo in ALGOS:
        for layout, M, N, K, split in ALGO_SHAPES:
            add(layout, M, N, K, split=split, ws=True, algo=algo)
        for M, N, K in ((8192, 384, 1536), (16384, 192, 192), (1000, 100, 384)):
            add("NT", M, N, K, algo=algo, **RES)
        add("NT", 8192, 384, 1536, algo=algo, **GELU)
        add("NT", 8192, 384, 1536, algo=algo, c="f32", res="bf16")
        add("NT", 8192, 384, 1536, algo=algo, **dict(RES, res_row_mod=-2))
    add("NT", 8192, 384, 1536, algo=1463, **RES)
    return out


def table():
    lines = []
    for label, g in cases():
        rc, name, ns = kernel_name(g)
        prc, v2, rows, pns = plan(g)
        lines.append(f"{label} | {name if rc == 0 else f'rc {rc} {name}'} | {ns} | {f'{v2} {rows} {pns}' if prc == 0 else f'rc {prc}'}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="library to question (default: the built csts_amd/libcsts_hip.so)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        env = {k: v for k, v in os.environ.items() if not k.startswith("CSTS_GEMM")}
        if a.lib:
            env["CSTS_HIP_LIB"] = os.path.abspath(a.lib)
        env["CSTS_HALF"] = "bf16"
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--out", a.out] if a.out else [])
        sys.exit(subprocess.run(cmd, env=env).returncode)
    text = "\n".join(table()) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
