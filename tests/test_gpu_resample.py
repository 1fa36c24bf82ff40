"""csts_resample_wav (csts_amd/csrc/resample.hip, inputs.resample_audio) element by element against the float64 restatement of
the rule (tests/resample_reference.py).  The inputs are generated in fp32 (or int16), so the reference sees the same numbers.

Rates 48000, 44100, 32000, 22050, 16000, 8000, 192000 Hz -> 24 kHz.  Lengths: 1, 2, 147 (all shorter than the filter: both zero
edges overlap), 1000, 4099 (several runs), and per rate the three shortest lengths whose n_out reaches RUN - 1, RUN and RUN + 1
(RUN = 256 outputs, one workgroup's run); a decimating ratio hits the three exactly, an interpolating one (n_out grows by more
than one per sample) the nearest length above.

Bound, per output, derived and not tuned: |y_gpu - y_ref| <= (K + C + 2) * 2^-24 * S with K the taps the output uses, C the
channels and S = sum |x[i] h[.]|: the bound of a K-term fp32 dot product in any order, plus the rounding of the fp32 tap and of
the C-term channel mean.  A sequential fp32 emulation on the CPU stays below 0.45 of it for every rate here."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import resample_reference as R  # noqa: E402
from csts_amd import inputs, lib  # noqa: E402

DEV = torch.device("cuda:0")
RATES = (48000, 44100, 32000, 22050, 16000, 8000, 192000)
RUN = lib.RESAMPLE_RUN
EPS = 2.0 ** -24
_REF = {}


def run_lengths(rate):
    """The shortest n whose n_out reaches RUN - 1, RUN, RUN + 1."""
    up, down = R.ratio(rate)
    return tuple(((t - 1) * down) // up + 1 for t in (RUN - 1, RUN, RUN + 1))


def case(rate, n, C=1, B=1, int16=False):
    """Seeded input on the CPU and its float64 reference (y, bound), computed once and left unchanged."""
    key = (rate, n, C, B, int16)
    if key not in _REF:
        g = torch.Generator().manual_seed(rate + 7 * n + C + 100 * B + int(int16))
        if int16:
            wav = torch.randint(-32768, 32768, (B, C, n), generator=g, dtype=torch.int16)
        else:
            wav = torch.randn(B, C, n, generator=g, dtype=torch.float32)
        h, up, down, half = R.design(rate)
        mono = R.downmix(wav.numpy())
        ys, bounds = [], []
        for b in range(B):
            y, K, S = R.resample(mono[b], h, up, down, half)
            ys.append(y)
            bounds.append((K + C + 2) * EPS * S)
        _REF[key] = (wav, np.stack(ys), np.stack(bounds))
    return _REF[key]


def judge(got, y, bound, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == y.shape, (what, got.shape, y.shape)
    err = np.abs(got.cpu().numpy().astype(np.float64) - y)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: {y.shape[-1]} outputs, largest error / bound {ratio:.3f}, largest error {float(err.max()):.3e}")
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("rate", RATES)
def test_every_output_against_float64(rate):
    up, down = R.ratio(rate)
    special = run_lengths(rate)
    reached = [R.out_len(n, up, down) for n in special]
    if down >= up:
        assert reached == [RUN - 1, RUN, RUN + 1]
    else:
        assert all(t <= r < t + up for t, r in zip((RUN - 1, RUN, RUN + 1), reached))
    for n in R.LENGTHS + special:
        wav, y, bound = case(rate, n)
        got = inputs.resample_audio(wav[0, 0].to(DEV), rate)
        judge(got, y[0], bound[0], f"{rate} Hz n {n}")
        assert got.shape[0] == lib.load().csts_resample_len(n, up, down)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("int16", [False, True])
def test_batch_channels_and_int16(rate, int16):
    n = 1000
    wav, y, bound = case(rate, n, C=2, B=3, int16=int16)
    x = wav.to(DEV)
    got = inputs.resample_audio(x, rate)
    judge(got, y, bound, f"{rate} Hz (3, 2, {n}) {'int16' if int16 else 'fp32'}")
    # the same call on the pre-averaged mono signal
    mono = (x.float() / 32768.0 if int16 else x).mean(dim=1)
    pre = inputs.resample_audio(mono, rate)
    assert pre.shape == got.shape
    diff = np.abs(pre.cpu().numpy().astype(np.float64) - got.cpu().numpy().astype(np.float64))
    assert bool((diff <= bound).all())
    # (B, n) and (n,) shapes go the same way
    assert torch.equal(inputs.resample_audio(mono[1], rate), pre[1])


def test_the_model_rate_returns_the_argument_and_other_inputs_pass_through_the_kernel():
    x = torch.randn(2, 500, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert inputs.resample_audio(x, 24000) is x
    v = x[1]
    assert inputs.resample_audio(v, 24000) is v
    # stereo or int16 at the model's rate still needs the downmix / the scale: the filter of ratio 1/1 is a delta
    wav, y, bound = case(24000, 300, C=2, B=2)
    judge(inputs.resample_audio(wav.to(DEV), 24000), y, bound, "24000 Hz (2, 2, 300)")
    wav, y, bound = case(24000, 300, C=1, B=2, int16=True)
    judge(inputs.resample_audio(wav[:, 0].to(DEV), 24000), y, bound, "24000 Hz int16 (2, 300)")


@pytest.mark.parametrize("rate", [48000, 44100, 16000])
def test_repeated_calls_and_strided_views_give_the_same_bits(rate):
    wav, y, bound = case(rate, 4099, C=2, B=3)
    x = wav.to(DEV)
    first = inputs.resample_audio(x, rate)
    assert torch.equal(inputs.resample_audio(x, rate), first)
    wide = torch.zeros(3, 2, 2 * 4099, device=DEV)
    wide[:, :, ::2] = x
    view = wide[:, :, ::2]
    assert not view.is_contiguous() and torch.equal(inputs.resample_audio(view, rate), first)
    swapped = x.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not swapped.is_contiguous() and torch.equal(inputs.resample_audio(swapped, rate), first)
    judge(first, y, bound, f"{rate} Hz (3, 2, 4099)")


def test_filter_table_is_cached_per_device_and_matches_the_rule():
    taps, up, down, half = inputs.resample_filter(44100, device=DEV)
    assert (up, down, half) == (80, 147, 1470) and taps.dtype == torch.float32 and taps.shape == (2941,) and taps.device == DEV
    assert inputs.resample_filter(44100, device=DEV)[0] is taps
    assert np.array_equal(taps.cpu().numpy(), R.design(44100)[0].astype(np.float32))


def test_positions_past_2_to_31():
    """m * down passes 2^31 (44.1 kHz: down 147, beyond output 14.6 million): the head, the tail and the outputs around the
    crossing against float64; a 32-bit position would read the wrong samples there."""
    rate, n = 44100, 27_000_000
    h, up, down, half = R.design(rate)
    x = torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(11), device=DEV, dtype=torch.float32)
    got = inputs.resample_audio(x, rate)
    n_out = R.out_len(n, up, down)
    assert got.shape == (n_out,) and (n_out - 1) * down > 2 ** 31
    cross = 2 ** 31 // down
    m = np.concatenate([np.arange(0, 300), np.arange(cross - 300, cross + 300), np.arange(n_out - 300, n_out)])
    y, K, S = R.resample(x.cpu().numpy(), h, up, down, half, m=m)
    err = np.abs(got[torch.from_numpy(m).to(DEV)].cpu().numpy().astype(np.float64) - y)
    bound = (K + 1 + 2) * EPS * S
    print(f"positions past 2^31: largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()) and bool(torch.isfinite(got).all())
