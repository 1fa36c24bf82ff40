"""Recorded clips: the forecast datasets of the reference (slowfast/datasets/ego4d_avgaze_forecast.py and
aria_avgaze_forecast.py) from pre-decoded clips, resident on the device.

Layout under CSTS_AMD.DATA_ROOT (decoding is out of scope; tools/make_toy_dataset.py writes a small random one):
  train.csv, test.csv                         one clip per line, `<video>/<video>_t<start>_t<end>.mp4` (the reference's lists; the
                                              extension is ignored; val reads test.csv as the reference does)
  clips/<video>/<clip>.npz                    frames_u8 uint8 (N, H, W, 3), wav fp32 (n,) at 24 kHz [, fps]: what
                                              tools/predict.py --video reads.  [sample_rate]: the rate wav was recorded at;
                                              wav, floating or int16, (n,) or (C, n), is then brought to 24 kHz mono on the
                                              device (inputs.resample_audio) before the spectrogram.  Instead of frames_u8 a
                                              clip may hold frames_yuv uint8 (N, H * 3 / 2, W) with pixel_format "nv12" | "i420"
                                              [, yuv_matrix "bt601" | "bt709", yuv_full_range]: 4:2:0 pictures, kept and sampled
                                              in that format (half the bytes); a split is uniform in format, matrix and range
  gaze_frame_label/<video>_frame_label.csv    a header row, then one row per video frame; Ego4D keeps columns [1:] = x, y, type
                                              (ego4d_avgaze_forecast.py:121-122), Aria columns [2:] (aria_avgaze_forecast.py:115)
A clip's first label row is start * DATA.TARGET_FPS.

ClipStore reads a split once and keeps, per clip, the observed frames (the first 86 of 150, Ego4D; the first 60 of 100, Aria --
later frames are never model input) and ONE log-power spectrogram (inputs.stft_logpower); it packs them, and every label row,
into three arenas on the device.  ClipLoader.batch builds the per-clip tables on the host with numpy (clip_rule restates the
datasets' __getitem__), copies ONE small table to the device and assembles the batch there in one launch per stage
(inputs.batch_params, batch_sample, audio_gather, a label gather, gaze_heatmaps).  plan_epoch is the sampler."""
from __future__ import annotations

import csv
import os

import numpy as np
import torch

from . import inputs
from . import lib as L
from .infer import AUDIO_WIDTH, plan_video

# dataset -> (frames of a clip the table below was written for, observed frames, first label column of the csv, aria)
FORECAST = {"ego4d_av_gaze_forecast": (150, 86, 1, False), "aria_av_gaze_forecast": (100, 60, 2, True)}
BUDGET_KEY = "CSTS_AMD.DATA_RESIDENT_GB"


def dataset_rule(name: str):
    """(segment, observed, first label column, aria) of a forecast dataset; the estimation datasets are not built yet."""
    key = str(name).lower()
    if key not in FORECAST:
        raise NotImplementedError(f"dataset {name!r}: recorded clips are built for the forecast datasets only "
                                  f"({', '.join(sorted(FORECAST))}); the estimation datasets are a follow-up")
    return FORECAST[key]


def _dataset_of(cfg, mode: str) -> str:
    if mode not in ("train", "val", "test"):
        raise ValueError(f"mode must be train, val or test, got {mode!r}")
    return str(cfg.TEST.DATASET if mode == "test" else cfg.TRAIN.DATASET)


def read_split(root: str, mode: str):
    """The clips of a split: [(video, clip, start second, end second)] from train.csv (train) or test.csv (val, test)."""
    path = os.path.join(root, "train.csv" if mode == "train" else "test.csv")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found: a data set holds train.csv and test.csv")
    clips = []
    with open(path) as f:
        for line in f.read().splitlines():
            line = line.strip()
            if not line:
                continue
            video, name = line.split("/")[-2:]
            name = os.path.splitext(name)[0]
            try:
                t0, t1 = (int(p[1:]) for p in name.split("_")[-2:])          # ego4d_avgaze_forecast.py:226-227
            except ValueError:
                raise ValueError(f"{path}: {line!r} is not <video>/<video>_t<start>_t<end>.mp4")
            clips.append((video, name, t0, t1))
    if not clips:
        raise ValueError(f"{path} lists no clip")
    return clips


def read_labels(path: str, first_col: int) -> np.ndarray:
    """gaze_frame_label csv -> float64 (rows, L): the header row dropped, columns [first_col:] kept."""
    with open(path) as f:
        rows = [list(map(float, row)) for i, row in enumerate(csv.reader(f)) if i > 0 and row]
    return np.array(rows, dtype=np.float64).reshape(len(rows), -1)[:, first_col:]


def clip_rule(cfg, mode: str, n_frames: int, cols: int, u: float = None):
    """What __getitem__ of the two forecast datasets picks for ONE clip of n_frames frames whose spectrogram has `cols`
    columns -> {"frames": int64 (T,) input frames, "label_rows": int64 (T,) label rows relative to the clip's first,
    "centers": int32 (T,) audio window centres, "observed", "usable": the trimmed column count (:215)}.

    train: frames = temporal_indices(observed, T, rate, -1, views, u=u) (random sampling in the observed part, u the variate);
    label frames = linspace(last + 1 [+ rate: aria], last + n_frames - observed, T).astype(int64) with last the last input frame
    (ego4d :230-235, aria :226-231); centres = round(frame / observed * usable) clipped to [128, usable - 1 - 128] (:216-218).
    val / test: window 0 of infer.plan_video(cfg, n_frames, cols=cols)."""
    segment, observed, _, aria = dataset_rule(_dataset_of(cfg, mode))
    n_frames, cols = int(n_frames), int(cols)
    T, rate = int(cfg.DATA.NUM_FRAMES), int(cfg.DATA.SAMPLING_RATE)
    usable = observed * cols // n_frames
    if mode != "train":
        if str(cfg.TEST.DATASET).lower() != _dataset_of(cfg, mode).lower():
            raise ValueError("TRAIN.DATASET and TEST.DATASET must name the same data set")
        plan = plan_video(cfg, n_frames, cols=cols)
        return {"frames": plan["frames_idx"][0].astype(np.int64), "label_rows": plan["target_idx"][0].astype(np.int64),
                "centers": plan["audio_centers"][0].astype(np.int32), "observed": plan["observed"], "usable": usable}
    if n_frames <= observed:
        raise ValueError(f"the clip has {n_frames} frames, {observed} are observed and at least one more is predicted")
    if usable < AUDIO_WIDTH + 1:
        raise ValueError(f"the observed part of the spectrogram has {usable} columns ({cols} for {n_frames} frames), an audio "
                         f"window needs {AUDIO_WIDTH + 1}")
    _, _, frames = inputs.temporal_indices(observed, T, rate, -1, int(cfg.TEST.NUM_ENSEMBLE_VIEWS), target_fps=cfg.DATA.TARGET_FPS,
                                           fps=cfg.DATA.TARGET_FPS, u=u)
    frames = frames.astype(np.int64)
    last = int(frames[-1])
    first = last + 1 + (rate if aria else 0)
    label_rows = np.linspace(first, last + n_frames - observed, T).astype(np.int64)
    half = AUDIO_WIDTH // 2
    centers = np.clip(np.rint(frames.astype(np.float64) / observed * usable).astype(np.int64), half, usable - 1 - half)
    return {"frames": frames, "label_rows": label_rows, "centers": centers.astype(np.int32), "observed": observed, "usable": usable}


def plan_epoch(n_clips: int, batch: int, world: int, rank: int, seed: int, epoch: int, train: bool, group_sizes=None):
    """The batches of one epoch for one rank -> a list of groups, each a list of int64 arrays of clip numbers.

    train: one permutation from numpy's default_rng((seed, epoch)), the same on every rank; rank r takes every world-th element
    from r on; the incomplete last batch is dropped.  val / test: the clips in order, rank r every world-th; the short last
    batch is kept.  group_sizes = (bytes of every clip, budget in bytes): the rank's batches are cut into consecutive groups
    whose clips fit the budget together (a batch that does not fit alone is an error); None: one group."""
    n_clips, batch, world, rank = int(n_clips), int(batch), int(world), int(rank)
    if n_clips < 1 or batch < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"bad plan: {n_clips} clips, batch {batch}, rank {rank} of {world}")
    order = np.random.default_rng((int(seed), int(epoch))).permutation(n_clips) if train else np.arange(n_clips)
    mine = order[rank::world].astype(np.int64)
    if train:
        # every rank runs the same number of steps (the gradient all-reduce needs them all)
        steps = (n_clips // world) // batch
        batches = [mine[i * batch:(i + 1) * batch] for i in range(steps)]
    else:
        batches = [mine[i:i + batch] for i in range(0, len(mine), batch)]
    if group_sizes is None:
        return [batches] if batches else []
    sizes, budget = np.asarray(group_sizes[0], dtype=np.int64), int(group_sizes[1])
    groups, cur, seen, used = [], [], set(), 0
    for ids in batches:
        new = {int(i) for i in ids} - seen
        need = int(sum(sizes[i] for i in new))
        if cur and used + need > budget:
            groups.append(cur)
            cur, seen, used = [], set(), 0
            new = {int(i) for i in ids}
            need = int(sum(sizes[i] for i in new))
        if need > budget:
            raise ValueError(f"one batch of {len(ids)} clips needs {need} bytes, the budget is {budget}")
        cur.append(ids)
        seen |= new
        used += need
    if cur:
        groups.append(cur)
    return groups


def clip_pictures(z, path: str, pixel_format=None, matrix=None, full_range=None, lead: int = 1):
    """The pictures of one clip npz (an open numpy.load, or a dict of arrays) -> (frames, H, W, (pixel_format, matrix,
    full_range)): frames_u8 uint8 (N, H, W, 3) as ("rgb24", "bt601", False), or frames_yuv uint8 (N, H * 3 / 2, W) with the entry
    pixel_format "nv12" | "i420" and the optional entries yuv_matrix (default "bt601") and yuv_full_range (default False).  The
    three arguments override the entries.  lead: the leading dimensions in front of a picture (1: (N, ...), 2: (B, T, ...)).
    ValueError for an npz holding both kinds or neither, or a bad entry."""
    dims = "(N" if lead == 1 else "(B, T"
    names = z.files if hasattr(z, "files") else list(z)
    if "frames_u8" in names and "frames_yuv" in names:
        raise ValueError(f"{path} holds both frames_u8 and frames_yuv: a clip holds its pictures once, in one format")
    if "frames_yuv" not in names:
        if "frames_u8" not in names:
            raise ValueError(f"{path} lacks frames_u8 (or frames_yuv with pixel_format): a clip holds its pictures")
        if pixel_format not in (None, "rgb24"):
            raise ValueError(f"{path} holds frames_u8, packed RGB: pixel format {pixel_format!r} needs frames_yuv")
        frames = z["frames_u8"]
        if frames.dtype != np.uint8 or frames.ndim != lead + 3 or frames.shape[-1] != 3:
            raise ValueError(f"{path}: frames_u8 must be uint8 {dims}, H, W, 3), got {frames.shape} {frames.dtype}")
        return frames, int(frames.shape[-3]), int(frames.shape[-2]), ("rgb24", "bt601", False)
    if pixel_format is None:
        if "pixel_format" not in names:
            raise ValueError(f"{path} holds frames_yuv without a pixel_format entry (\"nv12\" or \"i420\")")
        pixel_format = str(np.asarray(z["pixel_format"]).reshape(-1)[0])
    if matrix is None:
        matrix = str(np.asarray(z["yuv_matrix"]).reshape(-1)[0]) if "yuv_matrix" in names else "bt601"
    if full_range is None:
        full_range = bool(np.asarray(z["yuv_full_range"]).reshape(-1)[0]) if "yuv_full_range" in names else False
    if pixel_format == "rgb24":
        raise ValueError(f"{path}: frames_yuv holds 4:2:0 pictures, pixel_format must be \"nv12\" or \"i420\"")
    inputs.check_pixel_format(pixel_format, matrix, full_range)
    frames = z["frames_yuv"]
    if frames.dtype != np.uint8 or frames.ndim != lead + 2:
        raise ValueError(f"{path}: frames_yuv must be uint8 {dims}, H * 3 / 2, W), got {frames.shape} {frames.dtype}")
    try:
        H, W = inputs._yuv_hw(frames.shape, pixel_format, "frames_yuv")
    except ValueError as e:
        raise ValueError(f"{path}: {e}")
    return frames, H, W, (pixel_format, matrix, bool(full_range))


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


class ClipStore:
    """One split of a data set, read once: the observed frames, one spectrogram and the label rows of every listed clip.

    Host side: per clip the uint8 frames (observed part; packed RGB, or 4:2:0 as the split's pixel_format says), the fp32 spectrogram (nbins, cols), and the tables n_frames, H, W,
    cols, usable, first label row (in the label arena) and label rows of its video.  Device side: the label arena fp64 (rows, L)
    (always resident) and, after upload(ids), the frame arena (uint8, recordings back to back at any byte) and the spectrogram
    arena (fp32) of those clips with their tables {byte offset, N, H, W} and {float offset, row stride, usable columns}."""

    def __init__(self, cfg, split: str, device):
        root = str(getattr(cfg.CSTS_AMD, "DATA_ROOT", "") or "")
        if not root:
            raise ValueError("CSTS_AMD.DATA_ROOT is empty: recorded clips need the data set's directory")
        self.cfg, self.split, self.root = cfg, split, root
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.CstsError("ClipStore keeps its arenas on MI355X: it needs a GPU device (there is no CPU fallback)")
        self.dataset = _dataset_of(cfg, split)
        self.segment, self.observed, first_col, self.aria = dataset_rule(self.dataset)
        self.clips = read_split(root, split)
        fps = int(cfg.DATA.TARGET_FPS)
        videos, tables = {}, []
        for video, _, _, _ in self.clips:
            if video not in videos:
                path = os.path.join(root, "gaze_frame_label", f"{video}_frame_label.csv")
                if not os.path.exists(path):
                    raise FileNotFoundError(f"{path} not found: the gaze labels of video {video}")
                videos[video] = len(tables)
                tables.append(read_labels(path, first_col))
        ncol = {t.shape[1] for t in tables}
        if len(ncol) != 1 or min(ncol) < 2:
            raise ValueError(f"the label tables must share one column count >= 2, got {sorted(ncol)}")
        base = np.cumsum([0] + [t.shape[0] for t in tables])
        self.labels_host = np.concatenate(tables, axis=0)
        self.labels = torch.from_numpy(self.labels_host).to(self.device)
        n = len(self.clips)
        self.frames_host, self.spec_host = [], []
        self.n_frames, self.hw = np.zeros(n, np.int64), np.zeros((n, 2), np.int64)
        self.cols, self.usable = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.label_first, self.label_end = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.pixel_format, self.yuv_matrix, self.yuv_full_range = "rgb24", "bt601", False      # the first clip's, below
        for i, (video, name, t0, _) in enumerate(self.clips):
            path = os.path.join(root, "clips", video, name + ".npz")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path} not found: clip {video}/{name} is listed in the {split} split")
            with np.load(path) as z:
                missing = [k for k in ("frames_u8", "wav") if k not in z.files and (k == "wav" or "frames_yuv" not in z.files)]
                if missing:
                    raise ValueError(f"{path} lacks {missing}: a clip holds frames_u8 (or frames_yuv with pixel_format), wav and "
                                     "optionally fps")
                if "yuv_window" in z.files:
                    raise ValueError(f"{path} holds a yuv_window entry: the clip store packs tight 4:2:0 pictures only, repack the "
                                     "surfaces first (inputs.yuv_window)")
                frames, H, W, fmt = clip_pictures(z, path)
                wav = z["wav"]
                rate = np.asarray(z["sample_rate"]).reshape(-1) if "sample_rate" in z.files else None
            if frames.shape[0] <= self.observed:
                what = "frames_u8 must be uint8 (N" if fmt[0] == "rgb24" else f"frames_yuv ({fmt[0]}) must be uint8 (N"
                tail = "H, W, 3)" if fmt[0] == "rgb24" else "H * 3 / 2, W)"
                raise ValueError(f"{path}: {what} > {self.observed}, {tail}, got {frames.shape} {frames.dtype}")
            if i == 0:
                self.pixel_format, self.yuv_matrix, self.yuv_full_range = fmt
            elif fmt != (self.pixel_format, self.yuv_matrix, self.yuv_full_range):
                raise ValueError(f"{path}: clip {video}/{name} holds {fmt[0]} pictures (matrix {fmt[1]}, full range {fmt[2]}), the "
                                 f"split {self.pixel_format} (matrix {self.yuv_matrix}, full range {self.yuv_full_range}): a split is "
                                 "uniform in pixel format, matrix and range")
            self.n_frames[i], self.hw[i] = frames.shape[0], (H, W)
            self.frames_host.append(np.ascontiguousarray(frames[:self.observed]))
            if rate is None:
                wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).reshape(1, -1).to(self.device)
            else:
                if rate.size != 1 or float(rate[0]) != int(rate[0]) or int(rate[0]) < 1 or wav.ndim not in (1, 2):
                    raise ValueError(f"{path}: sample_rate must be one positive integer and wav (n,) or (C, n), got {rate.tolist()} "
                                     f"and {wav.shape}")
                wav = np.ascontiguousarray(wav, dtype=None if wav.dtype == np.int16 else np.float32)
                wav = inputs.resample_audio(torch.from_numpy(wav).reshape(1, -1, wav.shape[-1]).to(self.device), int(rate[0]))
            spec = inputs.stft_logpower(wav)
            self.spec_host.append(spec[0].cpu().numpy())
            self.cols[i] = spec.shape[2]
            self.usable[i] = self.observed * self.cols[i] // self.n_frames[i]
            if self.usable[i] < AUDIO_WIDTH + 1:
                raise ValueError(f"{path}: the observed part of the spectrogram has {self.usable[i]} columns, an audio window "
                                 f"needs {AUDIO_WIDTH + 1}")
            v = videos[video]
            self.label_first[i] = base[v] + t0 * fps
            self.label_end[i] = base[v + 1]
        self.nbins = self.spec_host[0].shape[0]
        self.frame_bytes = np.array([f.nbytes for f in self.frames_host], np.int64)
        self.spec_floats = np.array([s.size for s in self.spec_host], np.int64)
        self.clip_bytes = self.frame_bytes + 4 * self.spec_floats
        self.resident = None                  # clip numbers of the uploaded group
        self.slot = np.full(n, -1, np.int64)
        self.uploads = 0

    def __len__(self):
        return len(self.clips)

    def format_args(self):
        """The keywords that tell inputs.batch_sample the split's pixel format: {} for packed RGB."""
        if self.pixel_format == "rgb24":
            return {}
        return dict(pixel_format=self.pixel_format, matrix=self.yuv_matrix, full_range=self.yuv_full_range)

    def budget_bytes(self):
        """CSTS_AMD.DATA_RESIDENT_GB in bytes, or None when 0: the whole split is resident."""
        gb = float(getattr(self.cfg.CSTS_AMD, "DATA_RESIDENT_GB", 0) or 0)
        if gb < 0:
            raise ValueError(f"{BUDGET_KEY} must be >= 0, got {gb}")
        return int(gb * 2 ** 30) if gb > 0 else None

    def upload(self, ids=None):
        """Pack the arenas of the clips `ids` (default: all) on the device; a group already resident is kept."""
        ids = np.arange(len(self)) if ids is None else np.unique(np.asarray(ids, dtype=np.int64))
        if self.resident is not None and np.array_equal(ids, self.resident):
            return
        fbytes = _align(int(self.frame_bytes[ids].sum()), 16)
        sfloats = int(self.spec_floats[ids].sum())
        need = fbytes + 4 * sfloats
        budget = self.budget_bytes()
        # let go of the previous group before the next one is allocated
        self.arena = self.spec_arena = self.clips_dev = self.specs_dev = None
        if budget is None:
            free = torch.cuda.mem_get_info(self.device)[0]
            if need > free:
                raise RuntimeError(f"the {self.split} split needs {need / 2 ** 30:.2f} GiB on the device, {free / 2 ** 30:.2f} GiB "
                                   f"are free: set {BUDGET_KEY} to a budget and the epoch is uploaded in groups")
        host = torch.empty(fbytes, dtype=torch.uint8)
        spec = torch.empty(sfloats, dtype=torch.float32)
        self.clips_host = np.zeros((len(self), 4), np.int64)
        self.specs_host = np.zeros((len(self), 3), np.int64)
        self.slot[:] = -1
        off = soff = 0
        hv, sv = host.numpy(), spec.numpy()
        for k, i in enumerate(ids.tolist()):
            f, s = self.frames_host[i], self.spec_host[i]
            hv[off:off + f.nbytes] = f.reshape(-1)
            sv[soff:soff + s.size] = s.reshape(-1)
            self.clips_host[i] = (off, f.shape[0], self.hw[i, 0], self.hw[i, 1])
            self.specs_host[i] = (soff, s.shape[1], self.usable[i])
            self.slot[i] = k
            off += f.nbytes
            soff += s.size
        self.arena = host.to(self.device)
        self.spec_arena = spec.to(self.device)
        self.resident = ids
        self.uploads += 1


class ClipLoader:
    """Batches of one split.  epoch(e) yields them in plan_epoch's order (uploading each group first); batch(ids) assembles one.

    A batch is the dict train.synthetic_batch returns -- video fp32 (B, 3, T, S, S), audio fp32 (B, 1, T, S, S), labels_hm
    (B, T, S/4, S/4), labels fp64 (B, T, L) -- plus "clip_ids" int64 (B,) numpy (after replacement), "frames_idx" int32 (B, T) on
    the device, "params" int32 (B, 5) and "key" (the int64 (1,) device tensor of the spatial variates; None in val / test), so
    a test can rebuild the batch from the existing single-recording ops."""

    def __init__(self, store: ClipStore, mode: str = None, batch: int = 1, world: int = 1, rank: int = 0, seed: int = None):
        self.store, self.cfg = store, store.cfg
        self.mode = store.split if mode is None else mode
        self.train = self.mode == "train"
        self.batch_size, self.world, self.rank = int(batch), int(world), int(rank)
        self.seed = int(self.cfg.RNG_SEED if seed is None else seed)
        cfg = self.cfg
        self.T = int(cfg.DATA.NUM_FRAMES)
        self.S = int(cfg.DATA.TRAIN_CROP_SIZE if self.train else cfg.DATA.TEST_CROP_SIZE)
        if self.S > min(AUDIO_WIDTH, store.nbins):
            raise ValueError(f"crop size {self.S}: the audio input is S bins x S columns of a {store.nbins} x {AUDIO_WIDTH} window")
        self.replaced = 0
        self.rng = np.random.default_rng((self.seed, 0, self.rank))
        self._logged_groups = False

    def plan(self, epoch: int):
        budget = self.store.budget_bytes()
        sizes = None if budget is None else (self.store.clip_bytes, budget)
        try:
            return plan_epoch(len(self.store), self.batch_size, self.world, self.rank, self.seed, epoch, self.train, sizes)
        except ValueError as e:
            if budget is None:
                raise
            raise ValueError(f"{BUDGET_KEY}: {e}")

    def epoch(self, epoch: int, log=None):
        """Yield the batches of `epoch`.  log: a callable taking one dict (the driver's json_stats line), told once how the
        split is cut into groups when CSTS_AMD.DATA_RESIDENT_GB is set."""
        self.rng = np.random.default_rng((self.seed, int(epoch), self.rank, 1))
        groups = self.plan(epoch)
        if log is not None and self.store.budget_bytes() is not None and not self._logged_groups:
            self._logged_groups = True
            log({"_type": "data_groups", "split": self.mode, "groups": len(groups), "budget_gb": float(self.cfg.CSTS_AMD.DATA_RESIDENT_GB),
                 "clips": len(self.store)})
        for group in groups:
            self.store.upload(np.concatenate(group) if self.store.budget_bytes() is not None else None)
            for ids in group:
                yield self.batch(ids)

    def steps(self, epoch: int = 0) -> int:
        return sum(len(g) for g in self.plan(epoch))

    def _rule(self, i: int):
        st = self.store
        u = float(self.rng.random()) if self.train else None
        return clip_rule(self.cfg, self.mode, int(st.n_frames[i]), int(st.cols[i]), u=u)

    def table(self, ids):
        """The host half of batch(): -> (clip numbers after replacement, int64 (B, 7 + 3 T) table = clip row {byte offset, N, H,
        W}, spectrogram row {float offset, stride, usable}, T label rows (absolute, in the label arena), T input frames, T audio
        centres).  A train / val clip whose last label row lies past its video's label table is replaced by another resident clip
        drawn from the epoch generator (ego4d_avgaze_forecast.py:237-239); test clips are taken as they are (a missing row is an
        error there, as in the reference)."""
        st, T = self.store, self.T
        ids = np.asarray(ids, dtype=np.int64).copy()
        tab = np.zeros((len(ids), 7 + 3 * T), np.int64)
        for b in range(len(ids)):
            for _ in range(64):
                i = int(ids[b])
                if st.slot[i] < 0:
                    raise RuntimeError(f"clip {i} is not resident: upload its group first")
                r = self._rule(i)
                rows = st.label_first[i] + r["label_rows"]
                if rows[-1] < st.label_end[i]:
                    break
                if self.mode == "test":
                    raise ValueError(f"clip {'/'.join(st.clips[i][:2])}: label row {int(rows[-1] - st.label_first[i])} of the clip is "
                                     "past the video's label table")
                ids[b] = int(st.resident[self.rng.integers(len(st.resident))])
                self.replaced += 1
            else:
                raise RuntimeError("no resident clip has labels for all its target frames")
            tab[b, 0:4] = st.clips_host[i]
            tab[b, 4:7] = st.specs_host[i]
            tab[b, 7:7 + T] = rows
            tab[b, 7 + T:7 + 2 * T] = r["frames"]
            tab[b, 7 + 2 * T:] = r["centers"]
        return ids, tab

    def spatial_args(self):
        cfg = self.cfg
        if self.train:
            return dict(train=True, min_scale=int(cfg.DATA.TRAIN_JITTER_SCALES[0]), max_scale=int(cfg.DATA.TRAIN_JITTER_SCALES[1]),
                        random_flip=bool(cfg.DATA.RANDOM_FLIP), inverse_uniform=bool(cfg.DATA.INV_UNIFORM_SAMPLE))
        return dict(train=False, spatial_idx=1)

    def assemble(self, tab_dev: torch.Tensor, tab_host, key=None):
        """The device half of batch(): the table on the device (read by the kernels when they run: no host sync, so the whole of
        it can be captured in a graph and replayed after tab_dev and key are rewritten in place) -> the batch dict."""
        st, T, S, cfg = self.store, self.T, self.S, self.cfg
        clips = tab_dev[:, 0:4].contiguous()
        specs = tab_dev[:, 4:7].contiguous()
        rows = tab_dev[:, 7:7 + T]
        frames_idx = tab_dev[:, 7 + T:7 + 2 * T].to(torch.int32)
        centers = tab_dev[:, 7 + 2 * T:].to(torch.int32)
        labels = st.labels[rows]                                              # (B, T, L) fp64
        params, new_labels = inputs.batch_params(labels, clips, S, key=key, clips_host=tab_host[:, 0:4], **self.spatial_args())
        video = inputs.batch_sample(st.arena, clips, frames_idx, params, S, tab_host[:, 0:4], mean=tuple(cfg.DATA.MEAN),
                                    std=tuple(cfg.DATA.STD), **st.format_args())
        audio = inputs.audio_gather(st.spec_arena, specs, centers, st.nbins, tab_host[:, 4:7], AUDIO_WIDTH)
        if S != AUDIO_WIDTH or st.nbins != S:      # S frequency bins x S columns around each frame, as train.synthetic_batch cuts them
            o = (AUDIO_WIDTH - S) // 2
            audio = audio[:, :, :, :S, o:o + S].contiguous()
        return {"video": video, "audio": audio, "labels_hm": inputs.gaze_heatmaps(new_labels, H=S // 4, W=S // 4),
                "labels": new_labels, "frames_idx": frames_idx, "params": params, "key": key}

    def batch(self, ids, key=None):
        """Assemble the batch of the clips `ids` (their group must be resident).  key: the int64 (1,) device tensor of the spatial
        variates (train); None draws it from torch's device generator, as inputs.spatial_sampling does."""
        if self.store.resident is None:
            self.store.upload()
        ids, tab = self.table(ids)
        dev = self.store.device
        if self.train and key is None:
            key = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=dev)
        out = self.assemble(torch.from_numpy(tab).to(dev, non_blocking=True), tab, key if self.train else None)
        out["clip_ids"] = ids
        return out
