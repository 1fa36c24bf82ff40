"""MVIT.DROPOUT_RATE, host side (no GPU): the model builds with the knob and keeps the reference's parameter surface, bad rates
are rejected, and the library's host evaluation of the dropout mask function (csts_dropout_mask_host) equals a Philox4x32-10
restatement in numpy (numpy's own Philox is the 4x64 variant)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, k0, k1):
    """Philox4x32-10 over arrays of counters c = [c0, c1, c2, c3] (uint64 arrays holding 32-bit values)."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in c]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return [v.astype(np.uint32) for v in c]


def mask_numpy(key, site, first, count, p):
    """The documented mask: counter (lo32(e >> 2), hi32(e >> 2), site, 0), word e & 3, dropped iff word < floor(p * 2^32)."""
    e = np.arange(count, dtype=np.uint64) + np.uint64(first)
    blk = e >> np.uint64(2)
    zeros = np.zeros_like(blk)
    w = np.stack(philox4x32_10([blk & M32, blk >> np.uint64(32), zeros + np.uint64(site), zeros], key & 0xFFFFFFFF, key >> 32), 1)
    words = w[np.arange(count), (e & np.uint64(3)).astype(np.int64)]
    return (words < np.uint64(int(np.floor(p * 2.0 ** 32)))).astype(np.uint8)


def test_numpy_philox_known_answers():
    """The restatement itself against the Random123 known-answer vectors of philox4x32_10."""
    z = philox4x32_10([0, 0, 0, 0], 0, 0)
    assert [int(v) for v in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = philox4x32_10([0xFFFFFFFF] * 4, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in f] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    pi = philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], 0xA4093822, 0x299F31D0)
    assert [int(v) for v in pi] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_model_builds_with_dropout_rate_and_keeps_the_parameter_surface():
    from csts_amd.config import load_yaml
    from csts_amd.build import build_model
    m = build_model(load_yaml(YAML, ["NUM_GPUS", 0, "MVIT.DROPOUT_RATE", 0.1]))
    ref = json.load(open(os.path.join(GOLDEN, "manifest_T8_kldiv.json")))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref["entries"]
    assert m.drop_rate == 0.1
    m = build_model(load_yaml(YAML, ["NUM_GPUS", 0, "MVIT.DROPOUT_RATE", 0.1, "MODEL.LOSS_FUNC", "kldiv+egonce"]))
    ref = json.load(open(os.path.join(GOLDEN, "manifest_T8.json")))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref["entries"]
    # the documented site table: block i of the registration order owns sites 2 + 3i .. 4 + 3i
    from csts_amd.model import Block
    names = [n for n, mod in m.named_modules() if isinstance(mod, Block)]
    assert names == [f"blocks.{i}" for i in range(16)] + [f"blocks_audio.{i}" for i in range(4)] + \
        ["temporal_fusion", "spatial_fusion"] + [f"decode_block{i}" for i in range(1, 5)]
    assert [m.get_submodule(n).dropout_site for n in names] == [2 + 3 * i for i in range(len(names))]
    assert all(m.get_submodule(n).drop_rate == 0.1 for n in names)


@pytest.mark.parametrize("rate", [-0.1, 1.0])
def test_bad_dropout_rate_is_rejected(rate):
    from csts_amd.config import load_yaml
    from csts_amd.build import build_model
    with pytest.raises(ValueError, match="DROPOUT_RATE"):
        build_model(load_yaml(YAML, ["NUM_GPUS", 0, "MVIT.DROPOUT_RATE", rate]))


@pytest.mark.parametrize("p", [1e-3, 0.1, 0.5, 0.9])
def test_host_mask_entry_equals_numpy_philox(p):
    from csts_amd import ops
    cases = [(0x0123456789ABCDEF, 0, 0, 4096), (0xFFFFFFFFFFFFFFFF, 1, 3, 1001), (0x9ABCDEF012345678, 7, 12345, 77),
             (0x0000000100000002, 79, (1 << 32) - 5, 523), (0xDEADBEEFCAFEF00D, 2 ** 31 + 5, (1 << 40) + 6, 1030)]
    for key, site, first, count in cases:
        got = ops.dropout_mask_host(key, site, first, count, p)
        ref = mask_numpy(key, site, first, count, p)
        assert got.dtype == np.uint8 and got.shape == (count,)
        assert np.array_equal(got, ref), (hex(key), site, first, count, p)
    big = ops.dropout_mask_host(0x5555AAAA3333CCCC, 11, 0, 1 << 16, p)
    sigma = np.sqrt(p * (1 - p) / big.size)
    assert abs(float(big.mean()) - p) < 6 * sigma + 1e-12


def test_dropout_params():
    from csts_amd import ops
    assert ops.dropout_params(0.5) == (1 << 31, 2.0)
    thr, scale = ops.dropout_params(0.1)
    assert thr == 429496729 and scale == float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)))
