"""On-device spatial sampling, host side (no GPU): the library's rule (csts_spatial_rule_host), fed the variates the reference
drew, reproduces the reference's sizes, crop offsets, flips and labels (tests/golden/spatial_sampling.npz, written by
tools/gen_golden_spatial.py from slowfast/datasets/utils.py::spatial_sampling); the variates (csts_spatial_uniforms_host) are
Philox4x32-10 as documented; bad arguments are rejected; the config carries the reference's keys."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "spatial_sampling.npz")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
M32 = np.uint64(0xFFFFFFFF)


def fixture_cases():
    z = np.load(FIXTURE)
    meta = json.loads(str(z["cases"]))
    return [(m, {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}) for i, m in enumerate(meta)]


def rule_of(m, lab, u):
    from csts_amd import inputs
    return inputs.spatial_rule_host(lab[None], m["H"], m["W"], m["S"], train=m["train"], uniforms=u[None], min_scale=m["min_scale"],
                                    max_scale=m["max_scale"], spatial_idx=m["spatial_idx"], random_flip=m["random_flip"],
                                    inverse_uniform=m["inverse_uniform"])


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0]["name"])
def test_host_rule_reproduces_the_reference(case):
    m, d = case
    params, lab = rule_of(m, d["labels"], d["u"])
    assert params[0].tolist() == d["params"].tolist()
    assert np.abs(lab[0] - d["out_labels"]).max() <= 1e-12
    assert np.array_equal(lab[0][:, 2:], d["labels"][:, 2:])


def test_fixture_covers_the_rule():
    cases = {m["name"]: (m, d) for m, d in fixture_cases()}
    S = cases["square_eq_crop"][0]["S"]
    assert all(m["S"] == S for m, _ in cases.values())
    # both early returns: an S x S clip, labels returned untouched (outside [0, 1], not clipped; only x flipped)
    m, d = cases["square_eq_crop"]
    assert d["params"].tolist()[:4] == [S, S, 0, 0] and (d["labels"][:, :2] < 0).any() | (d["labels"][:, :2] > 1).any()
    x = 1 - d["labels"][:, 0] if d["params"][4] else d["labels"][:, 0]
    assert np.array_equal(d["out_labels"][:, 0], x) and np.array_equal(d["out_labels"][:, 1], d["labels"][:, 1])
    # jitter size == short side: no resize, the crop still moves
    m, d = cases["size_eq_short"]
    assert d["params"].tolist()[:2] == [m["H"], m["W"]]
    # the drop-one-end loop runs on x, on y, and on both
    for name, axes in (("spread_x", (0,)), ("spread_y", (1,)), ("spread_xy", (0, 1)), ("outside", (0, 1))):
        m, d = cases[name]
        for ax in axes:
            E = int(d["params"][1 - ax])
            g = d["labels"][:, ax] * E
            assert E > S and max(0, g.max() - S) > min(E - S, g.min()), (name, ax)
    assert {int(d["params"][4]) for m, d in cases.values() if m["train"]} == {0, 1}
    assert any(not m["random_flip"] for m in (c[0] for c in cases.values()))
    assert any(m["inverse_uniform"] for m in (c[0] for c in cases.values()))
    # test mode: idx 0 / 1 / 2 move along the long axis only, and labels are always clipped
    for orient, ax in (("landscape", 3), ("portrait", 2)):
        offs = [int(cases[f"test{i}_{orient}"][1]["params"][ax]) for i in range(3)]
        assert offs[0] == 0 < offs[1] < offs[2]
    assert all(((d["out_labels"][:, :2] >= 0) & (d["out_labels"][:, :2] <= 1)).all() for m, d in cases.values() if not m["train"])


def philox4x32_10(c, k0, k1):
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in c]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return [v.astype(np.uint64) for v in c]


def uniforms_numpy(key, first, count):
    """The documented variates: counters (lo32(b), hi32(b), 0x53504154, j), doubles ((a >> 5) 2^26 + (b >> 6)) 2^-53."""
    b = np.arange(count, dtype=np.uint64) + np.uint64(first)
    out = np.zeros((count, 4))
    for j in range(2):
        w = philox4x32_10([b & M32, b >> np.uint64(32), np.full_like(b, 0x53504154), np.full_like(b, j)], key & 0xFFFFFFFF, key >> 32)
        for h in range(2):
            a, c = w[2 * h], w[2 * h + 1]
            out[:, 2 * j + h] = ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (c >> np.uint64(6)).astype(np.float64)) / 2.0 ** 53
    return out


def test_numpy_philox_known_answers():
    assert [int(v) for v in philox4x32_10([0, 0, 0, 0], 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v) for v in philox4x32_10([0xFFFFFFFF] * 4, 0xFFFFFFFF, 0xFFFFFFFF)] == \
        [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    pi = philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], 0xA4093822, 0x299F31D0)
    assert [int(v) for v in pi] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_host_uniforms_equal_numpy_philox():
    from csts_amd import inputs
    for key, first, count in ((0, 0, 64), (0x0123456789ABCDEF, 5, 300), (0xFFFFFFFFFFFFFFFF, (1 << 32) - 3, 9),
                              (0xDEADBEEFCAFEF00D, (1 << 40) + 1, 17)):
        got = inputs.spatial_uniforms_host(key, first, count)
        assert np.array_equal(got, uniforms_numpy(key, first, count)), hex(key)
    u = inputs.spatial_uniforms_host(0x5555AAAA3333CCCC, 0, 1 << 14)
    assert (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 0.01
    # a known answer of the definition itself: the first variate of clip 0 under key 0
    w = philox4x32_10([0, 0, 0x53504154, 0], 0, 0)
    assert inputs.spatial_uniforms_host(0, 0, 1)[0, 0] == ((int(w[0]) >> 5) * 2 ** 26 + (int(w[1]) >> 6)) / 2.0 ** 53


def test_rule_edge_cases():
    from csts_amd import inputs
    # Python round() is half to even: min 256, max 257, u0 = 0.5 -> 256.5 -> 256 (no resize of a 256-short clip)
    lab = np.full((1, 2, 3), 0.5)
    p, _ = inputs.spatial_rule_host(lab, 256, 300, 224, train=True, uniforms=[[0.5, 0.5, 0.5, 0.9]], min_scale=256, max_scale=257)
    assert p[0, :2].tolist() == [256, 300]
    p, _ = inputs.spatial_rule_host(lab, 256, 300, 224, train=True, uniforms=[[0.5, 0.5, 0.5, 0.9]], min_scale=257, max_scale=258)
    assert p[0, :2].tolist() == [258, int(np.floor(300 / 256 * 258))]
    # the one point left outside [0, E]: the window nearest to it instead of the reference's empty max()
    lab = np.array([[[1.5, -0.5, 0.0]]])
    p, out = inputs.spatial_rule_host(lab, 64, 64, 32, train=True, uniforms=[[0.0, 0.3, 0.3, 0.9]], min_scale=48, max_scale=48)
    assert p[0].tolist() == [48, 48, 0, 16, 0] and out[0, 0, :2].tolist() == [1.0, 0.0]
    # test mode ignores the jitter range and the variates
    p, _ = inputs.spatial_rule_host(np.full((2, 4, 2), 0.5), 480, 640, 256, train=False, spatial_idx=1)
    assert p.tolist() == [[256, 341, 0, 43, 0]] * 2


def test_bad_arguments_are_rejected():
    from csts_amd import inputs
    from csts_amd.lib import CstsError
    f = torch.zeros(1, 4, 40, 40, 3, dtype=torch.uint8)
    lab = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match="below the crop"):
        inputs.spatial_sampling(f, lab, 32, train=True, min_scale=30, max_scale=40)
    with pytest.raises(ValueError, match="max_scale"):
        inputs.spatial_sampling(f, lab, 32, train=True, min_scale=36, max_scale=34)
    with pytest.raises(ValueError, match="T <= 64"):
        inputs.spatial_sampling(torch.zeros(1, 65, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 65, 2), 8, train=False)
    with pytest.raises(ValueError, match="uint8"):
        inputs.spatial_sampling(f.float(), lab, 32, train=False)
    with pytest.raises(ValueError, match="uint8"):
        inputs.spatial_sampling(f[0], lab, 32, train=False)
    with pytest.raises(ValueError, match="labels"):
        inputs.spatial_sampling(f, lab[0], 32, train=False)
    with pytest.raises(ValueError, match="labels"):
        inputs.spatial_sampling(f, lab.long(), 32, train=False)
    with pytest.raises(ValueError, match="labels"):
        inputs.spatial_sampling(f, lab[..., :1], 32, train=False)
    with pytest.raises(ValueError, match="spatial_idx"):
        inputs.spatial_sampling(f, lab, 32, train=False, spatial_idx=3)
    with pytest.raises(ValueError, match="params"):
        inputs.spatial_sample(f, torch.zeros(1, 5, dtype=torch.int64), 32)
    with pytest.raises(CstsError, match="GPU"):
        inputs.spatial_sampling(f, lab, 32, train=False)
    # the C entries check on their own
    with pytest.raises(CstsError, match="min_scale"):
        inputs.spatial_rule_host(np.zeros((1, 4, 3)), 40, 40, 32, train=True, uniforms=np.zeros((1, 4)), min_scale=31, max_scale=40)
    with pytest.raises(CstsError, match="T <= 64"):
        inputs.spatial_rule_host(np.zeros((1, 65, 3)), 40, 40, 32, train=False)
    with pytest.raises(CstsError, match="L >= 2"):
        inputs.spatial_rule_host(np.zeros((1, 4, 1)), 40, 40, 32, train=False)
    with pytest.raises(ValueError, match="uniforms"):
        inputs.spatial_rule_host(np.zeros((2, 4, 3)), 40, 40, 32, train=True, uniforms=np.zeros((1, 4)), min_scale=32, max_scale=40)


def test_config_keys_and_reference_defaults():
    from csts_amd.config import get_cfg, load_yaml
    from csts_amd import train as T
    c = get_cfg()
    assert c.DATA.RANDOM_FLIP is True and c.DATA.INV_UNIFORM_SAMPLE is False       # slowfast/config/defaults.py:485,488
    assert c.CSTS_AMD.SYNTHETIC_SOURCE_HW == []
    cfg = load_yaml(YAML)
    assert T.spatial_config(cfg, True) is None and T.spatial_config(cfg, False) is None
    cfg = load_yaml(YAML, ["CSTS_AMD.SYNTHETIC_SOURCE_HW", "[288,352]", "DATA.RANDOM_FLIP", "False"])
    tr, te = T.spatial_config(cfg, True), T.spatial_config(cfg, False)
    assert tr["source_hw"] == (288, 352) and tr["train"] is True and (tr["min_scale"], tr["max_scale"]) == (256, 288)
    assert tr["random_flip"] is False and tr["inverse_uniform"] is False
    assert te["train"] is False and te["spatial_idx"] == 1 and te["source_hw"] == (288, 352)
    with pytest.raises(ValueError, match="SYNTHETIC_SOURCE_HW"):
        T.spatial_config(load_yaml(YAML, ["CSTS_AMD.SYNTHETIC_SOURCE_HW", "[288]"]), True)
