"""ops._wg_plan, the host planner of the grouped weight-gradient launches (CPU only): which (layer, tile, token range) every work
item gets, where it sits in the table (position slot * 8 + xcd) and which slots are padding.  A lost or duplicated item is a
silently wrong gradient, so every plan below is checked for exact coverage, alignment, XCD placement and item fields."""
import os
from collections import defaultdict

import numpy as np
import pytest

from csts_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (tile rows, tile cols, token chunk, strided, token granule the class needs)
CLASSES = {
    "192": (192, 384, 8192, False, 64),
    "96": (96, 96, 4096, False, 16),
    "96s": (96, 96, 4096, True, 16),
    "256": (256, 128, 8192, False, 1),
    "128": (128, 128, 8192, False, 1),
}


def _b4_step():
    """The problem list of one b = 4 train step (tools/wgrad_problems_b4.txt: dtype tokens N K ...), split by tile class the
    way ops.flush_wgrads splits it with the default switches."""
    out = defaultdict(list)
    with open(os.path.join(ROOT, "tools", "wgrad_problems_b4.txt")) as f:
        for line in f:
            dt, tokens, N, K = line.split()[:4]
            tokens, N, K = int(tokens), int(N), int(K)
            if dt == "f32":
                cls = "128f"
            elif N % 192 == 0 and K % 384 == 0 and tokens % 64 == 0:
                cls = "192"
            elif N % 96 == 0 and K % 96 == 0 and tokens % 16 == 0 and min(N, K) >= 96:
                cls = "96"
            else:
                cls = "256" if N % 256 == 0 else "128"
            out[cls].append((tokens, N, K))
            assert ops._wg_class(dt == "f32", tokens, N, K).name == cls, line       # ops' own table names the same class
    return out


# problems per tile class that flush_wgrads made of tools/wgrad_problems_b4.txt before the class table existed (counted there
# through its _wg_plan calls and launches, default switches)
B4_CLASS_COUNTS = {"192": 79, "96": 30, "256": 0, "128": 0, "128f": 4}


def check_plan(sig, cls):
    rows, cols, CH, strided, gran = CLASSES[cls]
    tmpl, valid, pidx, chunk, n_items, CHs = ops._wg_plan(tuple(sig), rows, cols, CH, strided=strided)
    assert len(tmpl) == n_items and n_items % 8 == 0 and n_items > 0
    assert valid.dtype == bool and int(valid.sum()) == len(pidx) == len(chunk)
    assert CHs == [CH] * len(sig)
    # padding: every slot without a problem is all zeros (the kernels see A == NULL and skip it)
    assert not tmpl[~valid].tobytes().strip(b"\0")
    assert (tmpl["A"] == 0).all() and (tmpl["B"] == 0).all() and (tmpl["C"] == 0).all() and (tmpl["colsum"] == 0).all()
    pos = np.nonzero(valid)[0]
    it = tmpl[valid]
    tiles = defaultdict(list)            # (problem, m0, n0) -> [(kbeg, kend, step, chunk)]
    groups = defaultdict(set)            # (problem, chunk) -> XCDs its items sit on
    for k in range(len(pos)):
        p, c = int(pidx[k]), int(chunk[k])
        tokens, N, K = sig[p]
        e = it[k]
        # M, N, lda, ldb, ldc match the problem (96 class: M carries the stage step)
        assert (e["N"], e["lda"], e["ldb"], e["ldc"]) == (K, N, K, K), (cls, p, e)
        nch = -(-tokens // CH)
        if rows == 96:
            assert e["M"] == (nch if strided else 0), (cls, p, e)
        else:
            assert e["M"] == N, (cls, p, e)
        assert e["m0"] % rows == 0 and 0 <= e["m0"] < N and e["n0"] % cols == 0 and 0 <= e["n0"] < K
        assert 0 <= c < nch
        step = int(e["M"]) if strided else 1
        tiles[(p, int(e["m0"]), int(e["n0"]))].append((int(e["kbeg"]), int(e["kend"]), step, c))
        groups[(p, c)].add(int(pos[k]) % 8)
    # every tile of every problem, and nothing else
    want = {(p, m0, n0) for p, (tokens, N, K) in enumerate(sig) for m0 in range(0, N, rows) for n0 in range(0, K, cols)}
    assert set(tiles) == want, (cls, len(set(tiles) ^ want))
    for (p, m0, n0), rngs in tiles.items():
        tokens = sig[p][0]
        nch = -(-tokens // CH)
        assert sorted(r[3] for r in rngs) == list(range(nch)), (cls, p, m0, n0)       # one item per chunk
        if strided:
            nst = -(-tokens // 16)
            seen = np.zeros(nst, dtype=np.int64)
            for kb, ke, step, c in rngs:
                assert kb == 16 * c and ke == tokens and step == nch and kb % 16 == 0
                seen[np.arange(kb // 16, nst, step)] += 1
            assert (seen == 1).all(), (cls, p, m0, n0)           # the interleaved stages cover every 16-token stage exactly once
            continue
        cur = 0
        for kb, ke, step, c in sorted(rngs):                     # the token ranges partition [0, tokens) exactly once
            assert kb == cur and ke > kb and kb == c * CH, (cls, p, m0, n0, rngs)
            assert kb % gran == 0 and (ke - kb) % gran == 0, (cls, p, kb, ke)     # chunk boundaries and whole k-tiles
            cur = ke
        assert cur == tokens, (cls, p, m0, n0, rngs)
    # all items of one (layer, chunk) group sit on one XCD (index % 8)
    assert all(len(x) == 1 for x in groups.values()), cls
    # the lists are dense: an XCD's items come first, padding only after them
    for x in range(8):
        col = valid[x::8]
        assert not (col[1:] & ~col[:-1]).any(), (cls, x)
    # same plan object from the cache on a second call
    assert ops._wg_plan(tuple(sig), rows, cols, CH, strided=strided)[0] is tmpl
    return tmpl, valid


def test_b4_step_plans():
    """The real problem list of a b = 4 step, every tile class it reaches."""
    step = _b4_step()
    assert {k: len(step[k]) for k in B4_CLASS_COUNTS} == B4_CLASS_COUNTS
    assert step["192"] and step["96"] and step["128f"]
    check_plan(step["192"], "192")
    check_plan(step["96"], "96")
    check_plan(step["96"], "96s")
    check_plan(step["128f"], "128")
    if step["256"]:
        check_plan(step["256"], "256")
    if step["128"]:
        check_plan(step["128"], "128")
    # the 192 x 384 class of the step: 310 items (docstring of ops._wg_plan), 8 XCD lists of at most ceil(310 / 8) + a few
    tmpl, valid = check_plan(step["192"], "192")
    assert int(valid.sum()) == sum(-(-t // 8192) * (N // 192) * (K // 384) for t, N, K in step["192"])


EDGE = {
    "192": [
        [(8192, 192, 384)],                                      # a single problem, tokens == chunk
        [(8192 + 64, 1152, 384)],                                # one chunk + 64
        [(64, 192, 384), (128, 384, 768), (8192 * 3 + 192, 2304, 768)],
        [(2048 * (i % 5 + 1), 192 * (i % 3 + 1), 384 * (i % 2 + 1)) for i in range(23)],   # many groups over the 8 XCDs
    ],
    "96": [
        [(4096, 96, 96)],
        [(4096 + 16, 96, 288)],                                  # one chunk + 16: not a multiple of 64
        [(4112, 192, 384), (48, 96, 192), (4096 * 2 + 64, 288, 96)],
        [(16 * (37 * i + 5), 96 * (i % 4 + 1), 96 * (i % 3 + 1)) for i in range(19)],
    ],
    "256": [
        [(300, 256, 200)],
        [(8192 + 100, 512, 136)],
        [(8192 * 2, 256, 256), (999, 768, 8), (8200, 256, 72)] + [(256 + 8 * i, 256, 128) for i in range(12)],
    ],
    "128": [
        [(257, 200, 136)],
        [(8192, 8, 8)],
        [(8192 + 1, 72, 264), (9000, 136, 264), (300, 1000, 8)] + [(256 + 24 * i, 8 * (i + 1), 64) for i in range(14)],
    ],
}


@pytest.mark.parametrize("cls", ["192", "96", "96s", "256", "128"])
def test_edge_plans(cls):
    """A single problem, tokens equal to the chunk, one chunk + 64 (+ 16 for the 96 class: token counts that are multiples of 16
    only), ragged last chunks, and more (layer, chunk) groups than XCDs."""
    for sig in EDGE[cls.rstrip("s")]:
        check_plan(sig, cls)


def test_groups_spread_over_xcds():
    """More than 8 groups: every XCD gets work, and the longest list is at most one group longer than balance requires."""
    sig = [(8192, 192, 384)] * 16
    tmpl, valid = check_plan(sig, "192")
    per_xcd = [int(valid[x::8].sum()) for x in range(8)]
    assert per_xcd == [2] * 8 and len(tmpl) == 16
