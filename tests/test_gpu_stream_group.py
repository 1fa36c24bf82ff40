"""GazeStreamGroup against the composition of public pieces: every emitted window equals, bit for bit, its row of predict_batch
on the batch group_schedule names, each row built from that slot's whole recording by clip_sample at stream_window's frames and
audio_windows_at on stft_logpower of its whole waveform.  Random weights, bf16, the Ego4D forecast YAML, stride 9.  Three
recordings: slot 0: 104 frames of 64 x 80 with 83 200 samples; slot 1: 104 frames of 48 x 64 with 83 200 samples; slot 2: 95 frames
of 64 x 80 with 76 000 samples.  Slots 0 and 1 yield windows 0..2; slot 2 yields windows 0 and 1 (window 2 needs 104 frames)."""
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

from csts_amd import GazePredictor, GazeStreamGroup, group_schedule, inputs, stream_window  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402
from csts_amd.lib import CstsError  # noqa: E402
from csts_amd.stream import ring_sizes  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
STRIDE, PER = 9, 800
SHAPES = [(104, 64, 80), (104, 48, 64), (95, 64, 80)]
KEYS = ("points", "peak", "heatmaps", "rescaled")
COUNTERS = ("frames", "samples", "input_samples", "cols", "next_window", "dropped", "closed", "hw")


def _recording(n, H, W, seed, per=PER):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    return {"frames": frames, "wav": (0.1 * torch.randn(n * per, generator=g)).to(DEV)}


@pytest.fixture(scope="module")
def env():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    recs = [_recording(n, H, W, 40 + i) for i, (n, H, W) in enumerate(SHAPES)]
    for r in recs:
        r["spec"] = inputs.stft_logpower(r["wav"][None])[0]
    return {"cfg": cfg, "predictor": predictor, "recs": recs, "plan": predictor.stream_group(1, stride=STRIDE).plan}


def compose(e, batches, nb, recs=None, slices=False):
    """{(slot, window): outputs} of the batches (lists of (slot, window) rows, one predict_batch call each, padded to nb rows by
    repeating the last) from public pieces: every row from its own recording.  slices: cut the audio windows as
    spec[:, c - 128 : c + 128] (for centres audio_windows_at would clamp at the end of a spectrogram)."""
    predictor, plan = e["predictor"], e["plan"]
    recs = e["recs"] if recs is None else recs
    mean, std = tuple(e["cfg"].DATA.MEAN), tuple(e["cfg"].DATA.STD)
    out = {}
    for rows in batches:
        assert 1 <= len(rows) <= nb
        video, audio = [], []
        for i, w in rows + [rows[-1]] * (nb - len(rows)):
            win, frames, spec = stream_window(plan, w), recs[i]["frames"], recs[i]["spec"]
            idx = torch.from_numpy(win["frames_idx"].astype(np.int32))[None].to(DEV)
            params = torch.tensor([predictor._video_params_row(frames.shape[1], frames.shape[2])], dtype=torch.int32, device=DEV)
            video.append(inputs.clip_sample(frames, idx, params, 256, mean=mean, std=std))
            cen = win["audio_centers"]
            if slices:
                audio.append(torch.stack([spec[:, c - 128:c + 128] for c in cen.tolist()])[None, None])
            else:
                assert int(cen.min()) >= 128 and int(cen.max()) <= spec.shape[1] - 1 - 128      # audio_windows_at clamps nothing
                audio.append(inputs.audio_windows_at(spec, torch.from_numpy(cen.astype(np.int32))[None].to(DEV)))
        res = predictor.predict_batch({"video": torch.cat(video), "audio": torch.cat(audio)})
        for b, row in enumerate(rows):
            assert row not in out
            out[row] = {k: res[k][b] for k in KEYS}
    return out


def same(results, want):
    """results: {slot: [window dicts]} (or a list of them, merged) against compose's answer: the same windows, the same bits."""
    merged = {}
    for res in results if isinstance(results, list) else [results]:
        for i, rs in res.items():
            merged.setdefault(i, []).extend(rs)
    got = [(i, r["window"]) for i in sorted(merged) for r in merged[i]]
    assert got == sorted(want), (got, sorted(want))
    for i, rs in merged.items():
        for r in rs:
            assert r["stream"] == i
            for k in KEYS:
                assert torch.equal(r[k], want[(i, r["window"])][k]), (i, r["window"], k)


def _replay(e, group, ticks, recs=None, ran=None):
    """Push ticks of {slot: (frames, samples)} counts cut from the recordings, in order -> the list of push results.  ran: a list
    that receives the batches every push ran."""
    recs = e["recs"] if recs is None else recs
    ran = [] if ran is None else ran
    at = {}
    out = []
    for tick in ticks:
        pieces = {}
        for i, (k, m) in tick.items():
            fa, sa = at.get(i, (0, 0))
            pieces[i] = (recs[i]["frames"][fa:fa + k] if k else None, recs[i]["wav"][..., sa:sa + m] if m else None)
            at[i] = (fa + k, sa + m)
        out.append(group.push(pieces))
        assert sorted(out[-1]) == sorted(tick)
        ran.append(group.batches)
    return out


def _even_ticks(shapes, k=8, per=PER):
    ticks = []
    for a in range(0, max(n for n, _, _ in shapes), k):
        ticks.append({i: (min(k, n - a), min(k, n - a) * per) for i, (n, _, _) in enumerate(shapes) if a < n})
    return ticks


def test_even_ticks_equal_the_composition_group_schedule_names(env):
    group = env["predictor"].stream_group(3, stride=STRIDE, batch=2)
    assert isinstance(group, GazeStreamGroup)
    per_slot = ring_sizes(group.plan, 32, 256)
    assert group.capacity == dict(per_slot, streams=3, total_bytes=3 * (per_slot["crop_bytes"] + per_slot["spec_bytes"]))
    assert tuple(group._crops.shape) == (3, 118, 3, 256, 256) and tuple(group._spec.shape) == (3, 256, 832)
    ticks = _even_ticks(SHAPES)
    schedule = group_schedule(group.plan, ticks, 2)
    batches = [rows for tick in schedule for rows in tick]
    # 88 frames: window 0 of all three slots; 96: window 1; 104: window 2 of slots 0 and 1
    assert batches == [[(0, 0), (1, 0)], [(2, 0)], [(0, 1), (1, 1)], [(2, 1)], [(0, 2), (1, 2)]]
    ran = []
    results = _replay(env, group, ticks, ran=ran)
    assert ran == schedule                                        # push follows group_schedule, batch by batch
    for res, tick in zip(results, schedule):
        assert sorted((i, r["window"]) for i, rs in res.items() for r in rs) == sorted(row for rows in tick for row in rows)
    same(results, compose(env, batches, 2))
    r = results[10][1][0]
    assert r["window"] == 0 and r["frames_idx"].tolist() == stream_window(group.plan, 0)["frames_idx"].tolist()
    assert r["points"].shape == (8, 2) and r["heatmaps"].shape == (8, 64, 64)
    assert group.frames == [104, 104, 95] and group.samples == [83200, 83200, 76000] == group.input_samples
    assert group.next_window == [3, 3, 2] and group.hw == [(64, 80), (48, 64), (64, 80)]


def test_ragged_ticks_make_other_batches_and_each_equals_its_own_composition(env):
    group = env["predictor"].stream_group(3, stride=STRIDE, batch=2)
    # slot 0 frame by frame, slot 1 everything at once, slot 2 frame by frame with its audio a second ahead
    ticks, sent = [], 0
    for t in range(104):
        tick = {0: (1, PER)}
        if t == 0:
            tick[1] = (104, 104 * PER)
        if t < 95:
            m = min(31 * PER if t == 0 else PER, 95 * PER - sent)
            tick[2], sent = (1, m), sent + m
        ticks.append(tick)
    assert sum(tk[2][0] for tk in ticks if 2 in tk) == 95 and sent == 95 * PER and ticks[65][2] == (1, 0)
    schedule = group_schedule(group.plan, ticks, 2)
    batches = [rows for tick in schedule for rows in tick]
    # slot 1's push is worked off in steps of 32 frames inside tick 0: windows 0 and 1 after 96 frames, window 2 after 104
    assert schedule[0] == [[(1, 0), (1, 1)], [(1, 2)]]
    assert batches == [[(1, 0), (1, 1)], [(1, 2)], [(0, 0), (2, 0)], [(0, 1), (2, 1)], [(0, 2)]]
    ran = []
    results = _replay(env, group, ticks, ran=ran)
    assert ran == schedule
    same(results, compose(env, batches, 2))


def test_one_slot_batch_1_equals_a_gaze_stream_on_the_same_pushes(env):
    rec = env["recs"][0]
    group = env["predictor"].stream_group(1, stride=STRIDE, batch=1)
    single = env["predictor"].stream(stride=STRIDE, batch=1)
    a = 0
    got, want = [], []
    for k in [1, 5, 11, 32, 2, 40, 13]:
        frames, wav = rec["frames"][a:a + k], rec["wav"][a * PER:(a + k) * PER]
        got += group.push({0: (frames, wav)})[0]
        want += single.push(frames, wav)
        a += k
    assert a == 104 and [r["window"] for r in got] == [0, 1, 2] == [r["window"] for r in want]
    for x, y in zip(got, want):
        for k in KEYS:
            assert torch.equal(x[k], y[k]), (x["window"], k)
    assert (group.frames[0], group.samples[0], group.cols[0]) == (single.frames, single.samples, single.cols)


def test_input_rate_48000_equals_the_composition_on_the_resampled_waveforms(env):
    g = torch.Generator().manual_seed(77)
    recs = []
    for i in range(2):
        wav48 = (0.1 * torch.randn(104 * 1600, generator=g)).to(DEV)
        whole = inputs.resample_audio(wav48, 48000)
        recs.append({"frames": env["recs"][i]["frames"], "wav": wav48, "spec": inputs.stft_logpower(whole[None])[0]})
    group = env["predictor"].stream_group(2, stride=STRIDE, batch=2, input_rate=48000)
    ticks = _even_ticks(SHAPES[:2], per=1600)
    batches = [rows for tick in group_schedule(group.plan, ticks, 2, input_rate=48000) for rows in tick]
    assert batches == [[(0, 0), (1, 0)], [(0, 1), (1, 1)], [(0, 2), (1, 2)]]
    results = _replay(env, group, ticks, recs=recs)
    same(results, compose(env, batches, 2, recs=recs))
    assert group.input_samples == [104 * 1600] * 2 and all(83170 <= s <= 83200 for s in group.samples)
    assert not torch.equal(recs[0]["spec"], env["recs"][0]["spec"])


def test_close_and_reset(env):
    recs = env["recs"]
    cut = 68640 - 60            # window 0 reads 572 columns; the running stream has 571 after 68 580 samples, close() adds the 572nd
    group = env["predictor"].stream_group(3, stride=STRIDE, batch=2)
    first = group.push({i: (recs[i]["frames"][:86], recs[i]["wav"][:cut]) for i in range(3)})
    assert first == {0: [], 1: [], 2: []} and group.cols == [571] * 3
    # close(1): GazeStream.close's windows and dropped count for that recording, at the same batch size
    single = env["predictor"].stream(stride=STRIDE, batch=2)
    assert single.push(recs[1]["frames"][:86], recs[1]["wav"][:cut]) == []
    want = single.close()
    done = group.close(1)
    assert list(done) == [1] and [r["window"] for r in done[1]] == [0] == [r["window"] for r in want]
    for k in KEYS:
        assert torch.equal(done[1][0][k], want[0][k]), k
    assert group.closed == [False, True, False] and group.dropped == [0, single.dropped, 0] and single.dropped == 7
    assert group.cols == [571, 572, 571]
    with pytest.raises(ValueError, match="slot 1: the stream is closed"):
        group.push({0: (None, None), 1: (recs[1]["frames"][86:87], None)})
    with pytest.raises(ValueError, match="closed already"):
        group.close(1)
    # close(): the closing windows of slots 0 and 2 in ONE batch, each against the offline spectrogram of its cut waveform
    offline = [dict(r, spec=inputs.stft_logpower(r["wav"][None, :cut])[0]) for r in recs]
    assert offline[0]["spec"].shape[1] == 572
    done = group.close()
    assert sorted(done) == [0, 2] and group.closed == [True] * 3 and group.dropped == [7, 7, 7]
    same(done, compose(env, [[(0, 0), (2, 0)]], 2, recs=offline, slices=True))
    assert group.close() == {}
    # reset(1): another recording of another size into the slot, while the rings still hold the old one
    with pytest.raises(ValueError, match="close"):
        env["predictor"].stream_group(1, stride=STRIDE).reset(0)
    group.reset(1)
    assert group.closed == [True, False, True] and group.hw[1] is None
    assert (group.frames[1], group.samples[1], group.cols[1], group.next_window[1], group.dropped[1]) == (0, 0, 0, 0, 0)
    other = _recording(104, 40, 56, 90)
    other["spec"] = inputs.stft_logpower(other["wav"][None])[0]
    fresh = [None, other, None]
    ticks = [{1: (50, 60 * PER)}, {1: (54, 44 * PER)}]
    batches = [rows for tick in group_schedule(group.plan, ticks, 2) for rows in tick]
    assert batches == [[(1, 0), (1, 1)], [(1, 2)]]
    same(_replay(env, group, ticks, recs=fresh), compose(env, batches, 2, recs=fresh))
    assert group.hw[1] == (40, 56)


def _counters(group):
    return {k: list(getattr(group, k)) for k in COUNTERS}


def test_a_refused_tick_leaves_every_counter_of_every_slot_unchanged(env):
    recs = env["recs"]
    group = env["predictor"].stream_group(3, stride=STRIDE, batch=2, input_rate=24000)
    _replay(env, group, [{0: (8, 8 * PER), 1: (3, 0), 2: (0, 5 * PER)}])
    before = _counters(group)
    assert before["frames"] == [8, 3, 0] and before["samples"] == [8 * PER, 0, 5 * PER]
    quiet = torch.zeros(120 * 832, device=DEV)
    with pytest.raises(ValueError, match=r"^slot 2: .*832 columns"):           # slot 2 is stuck; slots 0 and 1 are fine
        group.push({0: (recs[0]["frames"][8:16], recs[0]["wav"][8 * PER:16 * PER]), 1: (recs[1]["frames"][3:4], None), 2: (None, quiet)})
    assert _counters(group) == before
    with pytest.raises(ValueError, match=r"^slot 1: .*fixed by the first push"):
        group.push({0: (recs[0]["frames"][8:16], None), 1: (recs[0]["frames"][:1], None)})
    with pytest.raises(ValueError, match=r"^slot 0: "):
        group.push({0: (recs[0]["frames"][8:16, :, :, :2], None)})
    with pytest.raises(CstsError, match=r"^slot 1: .*GPU tensors"):
        group.push({0: (recs[0]["frames"][8:16], None), 1: (recs[1]["frames"][3:4].cpu(), None)})
    with pytest.raises(CstsError, match=r"^slot 0: .*GPU tensors"):
        group.push([(0, None, recs[0]["wav"][:10].cpu())])
    with pytest.raises(ValueError, match="at most once"):
        group.push([(0, None, None), (0, None, None)])
    with pytest.raises(ValueError, match="slot"):
        group.push({3: (None, None)})
    assert _counters(group) == before
    # the tick goes through once the stuck slot pushes what its ring takes, as if the refused ones had never been sent
    res = group.push({0: (recs[0]["frames"][8:16], recs[0]["wav"][8 * PER:16 * PER]), 2: (None, quiet[:120 * 700])})
    assert res == {0: [], 2: []} and group.frames == [16, 3, 0] and group.samples == [16 * PER, 0, 5 * PER + 120 * 700]


def test_live_and_overlay_are_not_keywords_of_a_group(env):
    with pytest.raises(TypeError):
        env["predictor"].stream_group(2, live="hold")
    with pytest.raises(TypeError):
        env["predictor"].stream_group(2, overlay=True)
    with pytest.raises(TypeError):
        GazeStreamGroup(env["predictor"], 2, live="hold")
    with pytest.raises(ValueError, match="positive"):
        env["predictor"].stream_group(0)
