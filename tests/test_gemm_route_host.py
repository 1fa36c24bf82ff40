"""The routing of csts_gemm, pinned on the host: tools/gemm_route_table.py asks the built library (csts_gemm_kernel_name and
csts_gemm_plan, both host-only; made-up operand pointers) for a fixed list of problems -- the shapes of the replayed train step and
of the GPU tests under every epilogue form, either side of each heuristic edge, fp32 compute, misaligned operands, the
up-sampled residual, forced tiles and every forced algo on problems it does and does not apply to -- and every line must equal
tests/golden/gemm_routes.txt.  The fixture was taken from the library before launch, plan and name shared one route();
its forced-algo lines were regenerated with that change (the name is now the kernel the launch code starts, a forced algo
that csts_gemm rejects is rejected here too, and the plan reports the forced route).  A changed line means a changed heuristic:
regenerate the fixture on purpose (python tools/gemm_route_table.py --out tests/golden/gemm_routes.txt) and say why."""
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT


def test_gemm_routes_match_the_fixture(tmp_path):
    out = tmp_path / "routes.txt"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gemm_route_table.py"), "--out", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = out.read_text().splitlines()
    want = open(os.path.join(GOLDEN, "gemm_routes.txt")).read().splitlines()
    assert len(got) == len(want), (len(got), len(want))
    bad = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not bad, f"{len(bad)} of {len(want)} routes differ; first: line {bad[0][0]}\n  fixture: {bad[0][1]}\n  library: {bad[0][2]}"
