"""Host side of the grouped overlay launch (no GPU): overlay_group_table, the rule by which ops.group_gaze_overlay and
ops.group_points_source lay out their job table, against a brute-force map from workgroup number to (job, frame, band); the C-ABI
declarations of the three entry points; and the refusals the entries make from the host copy of the table before any launch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENTRY_POINTS = ("csts_group_gaze_overlay", "csts_group_gaze_overlay_yuv", "csts_group_points_source")
JOBS = [(3, 40, 52), (1, 33, 30), (2, 64, 80)]


def test_the_table_of_the_three_jobs():
    from csts_amd import overlay_group_table
    t = overlay_group_table(JOBS)
    assert t["first_row"].tolist() == [0, 3, 4] and t["rows"] == 6
    assert t["first_workgroup"].tolist() == [0, 6, 8] and t["grid"] == 12
    assert t["bands"].tolist() == [2, 2, 2]
    assert t["vector"].tolist() == [1, 0, 1]                       # W % 4 == 0 unless the caller knows better
    assert overlay_group_table(JOBS, [False, False, True])["vector"].tolist() == [0, 0, 1]
    for key in ("first_row", "first_workgroup", "bands", "vector"):
        assert t[key].dtype == np.int64
    assert overlay_group_table([(1, 32, 8)])["bands"].tolist() == [1]
    assert overlay_group_table([(1, 31, 8)])["bands"].tolist() == [1]
    assert overlay_group_table([(1, 1, 1)])["bands"].tolist() == [1]
    assert overlay_group_table([(5, 1080, 1088)])["grid"] == 5 * 34


@pytest.mark.parametrize("bad", [(0, 40, 52), (1, 0, 52), (1, 40, 0), (-1, 40, 52), (1, 40, -4)])
def test_a_job_without_frames_or_size_is_refused_by_name(bad):
    from csts_amd import overlay_group_table
    with pytest.raises(ValueError, match=r"^job 1: "):
        overlay_group_table([(3, 40, 52), bad, (2, 64, 80)])
    with pytest.raises(ValueError, match=r"^job 0: "):
        overlay_group_table([bad])


def test_a_vector_flag_needs_a_width_of_four_pixel_groups():
    from csts_amd import overlay_group_table
    with pytest.raises(ValueError, match=r"^job 1: .*W % 4"):
        overlay_group_table(JOBS, [True, True, True])
    with pytest.raises(ValueError, match="one flag per job"):
        overlay_group_table(JOBS, [True])


def _find(first, g):
    """The kernel's binary search, restated: the last job whose first workgroup is <= g."""
    lo, hi = 0, len(first) - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if first[mid] <= g else (lo, mid - 1)
    return lo


def test_the_binary_search_agrees_with_a_linear_scan_on_every_workgroup():
    from csts_amd import overlay_group_table
    rng = np.random.default_rng(20240229)
    for _ in range(50):
        n = int(rng.integers(1, 40))
        jobs = [(int(rng.integers(1, 6)), int(rng.integers(1, 200)), int(rng.integers(1, 300))) for _ in range(n)]
        t = overlay_group_table(jobs)
        brute = [(j, k, b) for j, (K, H, W) in enumerate(jobs) for k in range(K) for b in range(-(-H // 32))]
        assert len(brute) == t["grid"]
        first = t["first_workgroup"].tolist()
        for g, (j, k, b) in enumerate(brute):
            got = _find(first, g)
            local = g - first[got]
            assert (got, local // int(t["bands"][got]), local % int(t["bands"][got])) == (j, k, b), (jobs, g)
        # the same search over the first rows names the job of every row (group_points_source)
        rows = [j for j, (K, _, _) in enumerate(jobs) for _ in range(K)]
        assert [_find(t["first_row"].tolist(), p) for p in range(t["rows"])] == rows


def test_header_declares_and_binding_binds_the_entry_points():
    from csts_amd import lib
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name in lib.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for kind in ("bf16", "fp16"):
            assert hasattr(ctypes.CDLL(lib._PATHS[kind]), name), (kind, name)


def _table(rows):
    t = np.asarray(rows, dtype=np.int64)
    return t, t.ctypes.data


def test_the_entries_refuse_from_the_host_table_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    fake, far = 4096, 1 << 20

    def rgb(rows, jobs=fake):
        t, ptr = _table(rows)
        return h.csts_group_gaze_overlay(jobs, ptr, len(rows), fake, fake, 32, 8, 8, 0.4, 5, None)

    def yuv(rows, layout=1):
        t, ptr = _table(rows)
        return h.csts_group_gaze_overlay_yuv(fake, ptr, len(rows), fake, fake, 32, 8, 8, 0.4, 5, layout, 0, 0, None)

    # {src, dst, K, H, W, new h, new w, y0, x0, flip, first row, first workgroup, vector}
    a = [fake, fake, 3, 40, 52, 32, 41, 0, 4, 0, 0, 0, 1]                       # in place: legal
    assert rgb([a, [far, far + 1, 1, 33, 30, 35, 32, 1, 0, 0, 3, 6, 0]]) == -1  # out one byte into its own frames
    assert b"overlaps frames" in h.csts_last_error()
    assert rgb([a, [far, fake + 100, 1, 33, 30, 35, 32, 1, 0, 0, 3, 6, 0]]) == -1
    assert b"outputs of two jobs overlap" in h.csts_last_error()
    assert rgb([[far, 2 * far, 3, 40, 52, 32, 41, 0, 4, 0, 0, 0, 1], [2 * far, 3 * far, 1, 33, 30, 35, 32, 1, 0, 0, 3, 6, 0]]) == -1
    assert b"overlaps frames" in h.csts_last_error()                            # job 0 writes what job 1 reads
    assert rgb([[fake, far, 3, 40, 8196, 32, 41, 0, 4, 0, 0, 0, 1]]) == -1
    assert b"W <= 8192" in h.csts_last_error()
    assert rgb([[fake, far, 0, 40, 52, 32, 41, 0, 4, 0, 0, 0, 1]]) == -1
    assert rgb([[fake + 1, far, 3, 40, 52, 32, 41, 0, 4, 0, 0, 0, 1]]) == -1
    assert b"vector flag" in h.csts_last_error()
    assert rgb([[fake, far, 3, 40, 50, 32, 41, 0, 4, 0, 0, 0, 1]]) == -1        # W % 4
    assert rgb([a, [far, 2 * far, 1, 33, 30, 35, 32, 1, 0, 0, 2, 6, 0]]) == -1
    assert b"first row" in h.csts_last_error()
    assert rgb([a, [far, 2 * far, 1, 33, 30, 35, 32, 1, 0, 0, 3, 5, 0]]) == -1
    assert b"first workgroup" in h.csts_last_error()
    assert rgb([[0, far, 3, 40, 52, 32, 41, 0, 4, 0, 0, 0, 0]]) == -1
    assert h.csts_group_gaze_overlay(fake, None, 1, fake, fake, 32, 8, 8, 0.4, 5, None) == -1        # no host copy
    assert yuv([[fake, far, 3, 40, 52, 32, 41, 0, 4, 0, 0, 0, 0]]) == -1
    assert b"vector-path jobs only" in h.csts_last_error()
    assert yuv([[fake, far, 3, 41, 52, 32, 41, 0, 4, 0, 0, 0, 1]]) == -1
    assert b"even H, W" in h.csts_last_error()
    assert yuv([[fake, far, 3, 40, 52, 32, 41, 0, 4, 0, 0, 0, 1]], layout=3) == -1
    t, ptr = _table([[0, 0, 3, 40, 52, 32, 41, 0, 4, 0, 1, 0, 0]])
    assert h.csts_group_points_source(fake, ptr, 1, fake, 32, fake, fake, None) == -1
    assert b"first row" in h.csts_last_error()
    t, ptr = _table([[0, 0, 3, 40, 52, 0, 41, 0, 4, 0, 0, 0, 0]])
    assert h.csts_group_points_source(fake, ptr, 1, fake, 32, fake, fake, None) == -1
    assert b"params row" in h.csts_last_error()
