"""inputs.StreamResampler / csts_resample_stream against inputs.resample_audio of the whole waveform: bit for bit, for every cut.
The per-output arithmetic is csts_resample_wav's, so no tolerance is needed or allowed.  n = 20011 samples: several runs of 256
outputs at every rate, no multiple of anything."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import inputs, lib  # noqa: E402

DEV = torch.device("cuda:0")
RATES = (48000, 44100, 16000, 8000, 192000, 11025)
N = 20011


def cut_sizes(name, n, seed):
    if name == "one_piece":
        return [n]
    if name == "random":
        rng = np.random.default_rng(seed)
        sizes, left = [0, 1], n - 1                               # at least one empty piece and one of a single sample
        while left:
            sizes.append(min(int(rng.integers(0, 3001)), left))
            left -= sizes[-1]
        order = rng.permutation(len(sizes))
        return [sizes[i] for i in order]
    assert name == "sevens"                                       # pieces shorter than the filter, then the rest
    return [7] * 100 + [n - 700]


def stream(x, rate, sizes):
    """Push x (n,) or (C, n) in pieces of `sizes` -> (the pushes' outputs, close()'s, the resampler); checks the bookkeeping."""
    r = inputs.StreamResampler(rate)
    bound = 2 * r.half // r.up + 2
    outs, a = [], 0
    for m in sizes:
        want = r.count(m)
        y = r.push(x[..., a:a + m])
        a += m
        assert y.dtype == torch.float32 and y.shape == (want,), (m, want, y.shape)
        assert r.consumed == a and r.produced == inputs.resample_ready(a, r.up, r.down, r.half)
        assert r._tail.shape[-1] <= bound and r._tail.dtype == x.dtype and r._tail.shape[0] == r.channels
        assert r._tail_base + r._tail.shape[-1] == a
        outs.append(y)
    assert a == x.shape[-1]
    rest = r.close()
    assert r.closed and r.produced == -(-a * r.up // r.down)
    return outs, rest, r


@pytest.fixture(scope="module")
def wave():
    x = (0.1 * torch.randn(N, generator=torch.Generator().manual_seed(77))).to(DEV)
    return {"x": x, "whole": {rate: inputs.resample_audio(x, rate) for rate in RATES}}


@pytest.mark.parametrize("cut", ["one_piece", "random", "sevens"])
@pytest.mark.parametrize("rate", RATES)
def test_every_cut_gives_the_bits_of_the_whole_waveform(wave, rate, cut):
    sizes = cut_sizes(cut, N, rate)
    assert sum(sizes) == N and (cut != "random" or (0 in sizes and 1 in sizes and max(sizes) <= 3000))
    outs, rest, r = stream(wave["x"], rate, sizes)
    got = torch.cat(outs + [rest])
    assert got.shape == wave["whole"][rate].shape and torch.equal(got, wave["whole"][rate])
    assert 10 <= rest.numel() <= 30                               # what the open stream held back
    if cut == "sevens" and rate == 192000:
        assert all(y.numel() in (0, 1) for y in outs[:100])
    with pytest.raises(ValueError, match="closed"):
        r.push(wave["x"][:5])


def test_int16_stereo_is_downmixed_in_the_kernel():
    g = torch.Generator().manual_seed(78)
    x = torch.randint(-32768, 32768, (2, 5000), generator=g, dtype=torch.int16).to(DEV)
    whole = inputs.resample_audio(x[None], 44100)[0]
    outs, rest, r = stream(x, 44100, cut_sizes("random", 5000, 3))
    assert (r.channels, r.dtype) == (2, torch.int16)
    assert torch.equal(torch.cat(outs + [rest]), whole)
    assert not torch.equal(whole, inputs.resample_audio(x[None, :1], 44100)[0])      # the second channel matters


@pytest.mark.parametrize("rate", (48000, 44100, 8000))
@pytest.mark.parametrize("n", (1, 2, 147))
def test_streams_shorter_than_the_filter(rate, n):
    """One or two samples make no output final, so the pushes return nothing and close() returns everything.  147 samples are
    longer than the 48 kHz and 8 kHz filters and make 70 outputs final at 44.1 kHz: there the pushes return resample_ready(n)."""
    x =(0.1 * torch.randn(n, generator=torch.Generator().manual_seed(n))).to(DEV)
    sizes = [1] * n if n < 147 else [100, 0, 47]
    outs, rest, r = stream(x, rate, sizes)
    final = inputs.resample_ready(n, r.up, r.down, r.half)        # 0 for one or two samples: no output has all its inputs yet
    assert sum(y.numel() for y in outs) == final and (n == 147 or (final == 0 and all(y.numel() == 0 for y in outs)))
    assert rest.numel() == -(-n * r.up // r.down) - final > 0
    assert torch.equal(torch.cat(outs + [rest]), inputs.resample_audio(x, rate))


def test_pass_through_at_the_target_rate_and_refusals():
    x = (0.1 * torch.randn(300, generator=torch.Generator().manual_seed(5))).to(DEV)
    r = inputs.StreamResampler(24000)
    assert r.count(100, x[:100]) == 100
    assert r.push(x[:100]).data_ptr() == x.data_ptr() and r.push(x[100:]).data_ptr() == x[100:].data_ptr()   # untouched, no delay
    assert (r.consumed, r.produced) == (300, 300) and r.close().numel() == 0
    stereo = torch.stack([x, -0.5 * x])
    outs, rest, _ = stream(stereo, 24000, [120, 1, 179])          # stereo at 24 kHz goes through the 1/1 filter
    assert torch.equal(torch.cat(outs + [rest]), inputs.resample_audio(stereo[None], 24000)[0])
    assert inputs.StreamResampler(48000).close().numel() == 0     # never got a sample
    r = inputs.StreamResampler(48000)
    r.push(x[:50])
    for bad in (x[:50].to(torch.int16), torch.stack([x[:50], x[:50]]), x[:50].reshape(1, 1, 50), x[:50].to(torch.int32)):
        with pytest.raises(ValueError):
            r.push(bad)
    with pytest.raises((ValueError, lib.CstsError)):
        r.push(x[:50].cpu())
    assert (r.consumed, r.produced) == (50, inputs.resample_ready(50, 1, 2, 20))


def _call(h, buf, taps, out, *, C=1, length=None, x_base=0, n_total=-1, up=80, down=147, half=1470, m0, m1):
    length = buf.shape[-1] if length is None else length
    return h.csts_resample_stream(buf.data_ptr(), lib.WAV_F32, C, length, x_base, n_total, taps.data_ptr(), up, down, half, m0, m1,
                                  out.data_ptr(), None)


def test_64_bit_positions_through_the_c_abi():
    h = lib.load()
    taps, up, down, half = inputs.resample_filter(44100, device=DEV)
    assert (up, down, half) == (80, 147, 1470)
    x = (0.1 * torch.randn(6000, generator=torch.Generator().manual_seed(9))).to(DEV)
    near, far = torch.zeros(2700, device=DEV), torch.zeros(2700, device=DEV)
    assert _call(h, x, taps, near, m0=300, m1=3000) == 0
    shift = 1 << 26                                               # a whole number of filter periods: 147 inputs <-> 80 outputs
    assert 147 * shift > 1 << 33 and 80 * shift > 1 << 32
    assert _call(h, x, taps, far, x_base=147 * shift, m0=300 + 80 * shift, m1=3000 + 80 * shift) == 0
    torch.cuda.synchronize()
    assert torch.equal(near, far) and float(near.abs().max()) > 0
    assert torch.equal(near, inputs.resample_audio(x, 44100)[300:3000])    # neither call touches the zero edge


def test_refusals_with_real_device_buffers():
    h = lib.load()
    taps, up, down, half = inputs.resample_filter(44100, device=DEV)
    x = torch.ones(6000, device=DEV)
    out = torch.full((4000,), 7.0, device=DEV)
    ready = inputs.resample_ready(6000, up, down, half)
    total = -(-6000 * up // down)
    assert _call(h, x, taps, out, m0=300, m1=ready) == 0          # the largest open call is fine ...
    out.fill_(7.0)
    assert inputs.resample_first_input(100, up, down, half) == 166
    bad = [dict(m0=300, m1=ready + 1),                            # ... one more output is not final yet
           dict(x_base=167, length=5833, m0=100, m1=3000),        # output 100 reads from input ceil(13230 / 80) = 166 < x_base
           dict(n_total=6001, m0=300, m1=3000),                   # x_base + len != n_total at close
           dict(n_total=6000, m0=300, m1=total + 1)]              # m1 past ceil(n_total up / down)
    for kw in bad:
        assert _call(h, x[:kw.get("length", 6000)], taps, out, **kw) != 0, kw
        assert b"csts_resample_stream" in h.csts_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert _call(h, x, taps, out, n_total=6000, m0=300, m1=total) == 0     # and the closing call with the same buffer runs
    torch.cuda.synchronize()
    assert bool((out[:total - 300] != 7.0).all()) and bool((out[total - 300:] == 7.0).all())
