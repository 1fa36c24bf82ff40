"""Host side of the fusion attention maps: the float64 restatement of csts_audio_pixel_attn's rule (tests/attention_reference.py)
against the reference's own order of operations, the end-pixel extrema against the full lattice, the command line's refusal of
--attention with --video, and the exported symbol.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attention_reference as A  # noqa: E402

COLUMNS = sorted(A.CASES) + ["fixture"]


def _column(name):
    if name == "fixture":
        return A.fixture_column(), 8, 256
    return A.host_column(name), A.CASES[name][6], A.CASES[name][7]


@pytest.mark.parametrize("name", COLUMNS)
def test_restatement_agrees_with_the_reference_order(name):
    """Rescale the coarse map by the lattice extrema, then upsample == upsample, then rescale per frame (the reference): the
    quantised values differ by at most one step, and only on the close set, which stays under 1 % of the pixels."""
    column, T, S = _column(name)
    r = A.restate(column, T, S)
    heads = column.shape[1]
    want = A.reference_order(column, T, S)
    diff = np.abs(r["q"][:, :heads] - want)
    share = float(r["close"].mean())
    print(f"{name}: close share {share:.4%}, pixels off by one {int((diff == 1).sum())} of {diff.size}, by more {int((diff > 1).sum())}")
    assert share <= 0.01
    assert int(diff.max()) <= 1
    assert not (diff > 0)[~r["close"][:, :heads]].any()


@pytest.mark.parametrize("name", COLUMNS)
def test_end_pixels_give_the_lattice_extrema_exactly(name):
    column, T, S = _column(name)
    m = A.mix_time(A.head_mean(column), T)
    lo, hi = A.lattice_range(m, S)
    elo, ehi = A.end_pixel_range(m, S)
    assert np.array_equal(lo, elo) and np.array_equal(hi, ehi)
    # the lattice never reaches a cell centre: its extrema lie inside the coarse map's own
    assert (hi <= m.max(axis=(-2, -1))).all() and (lo >= m.min(axis=(-2, -1))).all()
    h, w = m.shape[-2:]
    assert len(A.end_pixels(S, h)) <= 2 * h and len(A.end_pixels(S, w)) <= 2 * w


def test_time_identity_mixes_nothing():
    column, T, _ = _column("time_identity")
    assert np.array_equal(A.mix_time(column, T), column)


def test_cli_rejects_attention_on_a_whole_recording(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--attention", "--video", "x", "--out",
                        str(tmp_path / "o.npz")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and p.stdout.strip() == ""
    assert "--attention" in p.stderr and "--video" in p.stderr and "not defined yet" in p.stderr
    assert not (tmp_path / "o.npz").exists()


def test_library_exports_and_binds_the_entry():
    from csts_amd import lib
    assert "csts_audio_pixel_attn" in lib.SYMBOLS
    handle = lib.load()
    assert hasattr(handle, "csts_audio_pixel_attn")
    with open(os.path.join(ROOT, "include", "csts_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint csts_audio_pixel_attn\(", hdr)
    import csts_amd
    assert csts_amd.audio_pixel_attn is csts_amd.ops.audio_pixel_attn
