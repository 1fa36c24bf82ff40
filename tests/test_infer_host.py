"""Host side of the inference path (no GPU): the C ABI declares and exports csts_gaze_decode, load_test_checkpoint follows the
reference's TEST.CHECKPOINT_FILE_PATH rule (slowfast/utils/checkpoint.py:579-614, first and last branch), and the public entry
points refuse CPU tensors loudly instead of falling back."""
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")


class Tiny(torch.nn.Module):
    """The module of test_checkpoint_wire_format_reads_reference_written_pyth (tests/test_cpu_host.py)."""

    def __init__(self, T, nout):
        super().__init__()
        self.pos_embed_spatial = torch.nn.Parameter(torch.zeros(1, 16, 8))
        self.pos_embed_temporal = torch.nn.Parameter(torch.zeros(1, T, 8))
        self.blocks = torch.nn.ModuleList([torch.nn.Linear(8, 8) for _ in range(2)])
        self.head = torch.nn.Linear(8, nout)


def _tiny_before():
    g = np.load(os.path.join(GOLDEN, "ref_checkpoint_loaded.npz"))
    dst = Tiny(8, 5)
    dst.load_state_dict({k: torch.from_numpy(g["before__" + k.replace(".", "__")]) for k in dst.state_dict()})
    return dst, g


def test_gaze_decode_is_declared_bound_and_exported():
    from csts_amd import lib
    assert "csts_gaze_decode" in lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert re.search(r"\bint\s+csts_gaze_decode\s*\(", hdr)
    m = re.search(r"#define CSTS_GAZE_DECODE_MAX_HW (\d+)", hdr)
    assert m and int(m.group(1)) >= 4096                     # 64 x 64 heat maps of the 256^2 crop fit the register budget
    handle = lib.load()
    assert hasattr(handle, "csts_gaze_decode") and handle.csts_abi_version() == lib.ABI_VERSION


def test_gaze_decode_launch_checks_need_no_gpu():
    """Argument validation happens on the host before the launch: -1 and a message."""
    from csts_amd import lib
    h = lib.load()
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    max_hw = int(re.search(r"#define CSTS_GAZE_DECODE_MAX_HW (\d+)", hdr).group(1))
    fake = 4096                                              # never dereferenced: every call below fails its checks
    assert h.csts_gaze_decode(None, lib.F32, 1, 64, 64, 2.0, fake, None, None, None, None) == -1
    assert h.csts_gaze_decode(fake, lib.F32, 0, 64, 64, 2.0, fake, None, None, None, None) == -1
    assert b"frames" in h.csts_last_error()
    assert h.csts_gaze_decode(fake, lib.F32, 1, 1, max_hw + 1, 2.0, fake, None, None, None, None) == -1
    assert b"CSTS_GAZE_DECODE_MAX_HW" in h.csts_last_error()
    assert h.csts_gaze_decode(fake, lib.F32, 1, 64, 64, 0.0, fake, None, None, None, None) == -1
    assert h.csts_gaze_decode(fake, 7, 1, 64, 64, 2.0, fake, None, None, None, None) == -1


def test_load_test_checkpoint_loads_the_named_file():
    from csts_amd import checkpoint as ck
    from csts_amd.config import load_yaml
    cfg = load_yaml(YAML, ["NUM_GPUS", 0, "TEST.CHECKPOINT_FILE_PATH", os.path.join(GOLDEN, "ref_checkpoint_epoch_00007.pyth")])
    dst, g = _tiny_before()
    head_before = {k: v.clone() for k, v in dst.head.state_dict().items()}
    assert ck.load_test_checkpoint(cfg, dst) is None
    for k, v in dst.state_dict().items():
        assert torch.allclose(v, torch.from_numpy(g[k.replace(".", "__")]), atol=1e-7), k
    assert any(not torch.equal(v, torch.from_numpy(g["before__" + k.replace(".", "__")])) for k, v in dst.state_dict().items())
    for k, v in dst.head.state_dict().items():               # shape mismatch: left untouched, like the reference
        assert torch.equal(v, head_before[k])


def test_load_test_checkpoint_without_the_key_warns_and_leaves_the_model(caplog):
    from csts_amd import checkpoint as ck
    from csts_amd.config import load_yaml
    cfg = load_yaml(YAML, ["NUM_GPUS", 0])
    assert cfg.TEST.CHECKPOINT_FILE_PATH == ""
    dst, _ = _tiny_before()
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    with caplog.at_level(logging.WARNING, logger="csts_amd"):
        ck.load_test_checkpoint(cfg, dst)
    assert all(torch.equal(v, before[k]) for k, v in dst.state_dict().items())
    msgs = [r for r in caplog.records if r.levelno == logging.WARNING and "random initialization, only for debugging" in r.getMessage()]
    assert len(msgs) == 1


def test_load_test_checkpoint_with_a_missing_file_asserts(tmp_path):
    from csts_amd import checkpoint as ck
    from csts_amd.config import load_yaml
    cfg = load_yaml(YAML, ["NUM_GPUS", 0, "TEST.CHECKPOINT_FILE_PATH", str(tmp_path / "nope.pyth")])
    dst, _ = _tiny_before()
    with pytest.raises(AssertionError, match="not found"):
        ck.load_test_checkpoint(cfg, dst)


def test_inference_entry_points_refuse_cpu_tensors():
    import csts_amd
    from csts_amd import ops
    from csts_amd.config import load_yaml
    from csts_amd.infer import GazePredictor, GraphedEvalStep
    from csts_amd.lib import CstsError
    assert csts_amd.GazePredictor is GazePredictor and csts_amd.GraphedEvalStep is GraphedEvalStep
    with pytest.raises(CstsError):
        ops.gaze_decode(torch.zeros(1, 1, 2, 8, 8))
    cfg = load_yaml(YAML, ["NUM_GPUS", 1])
    with pytest.raises(CstsError):
        GazePredictor(cfg, device="cpu")
    shell = GazePredictor.__new__(GazePredictor)             # the input checks come before any use of the model
    with pytest.raises(CstsError):
        shell.predict(torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 100), torch.zeros(1, 2), 2.0)
    with pytest.raises(CstsError):
        shell.predict_batch({"video": torch.zeros(1, 3, 2, 8, 8), "audio": torch.zeros(1, 1, 2, 8, 8)})
    with pytest.raises(CstsError):
        GraphedEvalStep(cfg, torch.nn.Identity(), {"video": torch.zeros(1, 3, 2, 8, 8), "audio": torch.zeros(1, 1, 2, 8, 8)})
