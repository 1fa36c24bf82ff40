"""Evaluation metric of the gaze heat maps on the device: ``adaptive_f1`` with the reference's name, arguments and return
value (slowfast/utils/metrics.py:9-74), computed by csts_adaptive_f1 without the (n_thresholds, B, T, H, W) temporaries
of the reference.  ``rescale=True`` folds in the per-frame min-max rescale its callers apply first
(tools/test_avgaze_net.py:66-68, tools/train_avgaze_net.py:125-127)."""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L

_FIXATION_0 = ("ego4dgaze", "ego4dgaze_forecast", "ego4d_av_gaze", "ego4d_av_gaze_forecast", "aria_gaze",
               "aria_gaze_forecast", "aria_av_gaze", "aria_av_gaze_forecast")


def thresholds_for(dataset: str) -> np.ndarray:
    """metrics.py:35-43: the search space depends on the dataset."""
    if "forecast" in dataset and "aria" not in dataset:
        return np.linspace(0.01, 0.07, 31)
    if "forecast" in dataset and "aria" in dataset:
        return np.linspace(0.0, 0.02, 21)
    return np.linspace(0, 0.02, 11)


def adaptive_f1(preds, labels_hm, labels, dataset, rescale: bool = False):
    """preds (B, 1, T, H, W) heat maps (already min-max rescaled unless rescale=True), labels_hm (B, T, H, W),
    labels (B, T, 3) with the gaze type in [..., 2].  Returns (f1, recall, precision, threshold) as Python floats."""
    if not preds.is_cuda:
        raise L.CstsError("csts_amd.metrics.adaptive_f1 runs on MI355X only: inputs must be GPU tensors")
    if dataset == "egteagaze":
        fixation_idx = 1
    elif dataset in _FIXATION_0:
        fixation_idx = 0
    else:
        raise NotImplementedError(f"Metrics of {dataset} is not implemented.")
    thr = thresholds_for(dataset)
    dev = preds.device
    p = preds.detach().squeeze(1).contiguous().float()
    q = labels_hm.detach().contiguous().float()
    B, T, H, W = q.shape
    assert p.shape == q.shape, (p.shape, q.shape)
    tracked = (labels.detach().reshape(B * T, -1)[:, 2] == fixation_idx).to(torch.uint8).contiguous()
    thr_d = torch.tensor(thr.astype(np.float32), device=dev)      # torch compares an fp32 tensor with the scalar in fp32
    out = torch.empty(4, dtype=torch.float32, device=dev)
    lib = L.load()
    ws = torch.empty(max(int(lib.csts_adaptive_f1_workspace(B * T, len(thr))), 16), dtype=torch.uint8, device=dev)
    L.check(lib.csts_adaptive_f1(p.data_ptr(), q.data_ptr(), tracked.data_ptr(), thr_d.data_ptr(), len(thr), B * T, H * W,
                                 1 if rescale else 0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream), "csts_adaptive_f1")
    f1, rec, prec, idx = out.cpu().tolist()
    return float(f1), float(rec), float(prec), thr[int(idx)]


def fixation_index(dataset: str) -> int:
    """metrics.py:56-62: the gaze type whose frames count."""
    if dataset == "egteagaze":
        return 1
    if dataset in _FIXATION_0:
        return 0
    raise NotImplementedError(f"Metrics of {dataset} is not implemented.")


_MODES = ("train", "val", "test")
_WEIGHT_TYPE = 1      # meters.py:87-88,409-410: ValGazeMeter / TestGazeMeter weight a batch by its frames with labels[:, 2] == 1


class _MeterReader:
    """Reading side of a gaze-meter state buffer (layout: include/csts_hip.h, "gaze meters").  ``_state_host()`` returns the
    buffer as host bytes; it is the only place a device meter copies to the host."""

    def _fields(self):
        raw = np.ascontiguousarray(self._state_host()).view(np.uint8)
        n, w = len(self.thresholds), self.window
        hdr = raw[:16].view(np.int64)
        tot = raw[16:40].view(np.float64)
        sums = raw[40:40 + 16 * n].view(np.float64).reshape(2, n)
        ring = raw[40 + 16 * n:40 + 16 * n + 16 * w].view(np.float32).reshape(w, 4)
        return int(hdr[0]), int(hdr[1]), tot, sums, ring

    def iterations(self) -> int:
        return self._fields()[0]

    def last_batch(self):
        """(f1, recall, precision, threshold) of the latest batch: what adaptive_f1 returns for it."""
        it, _, _, _, ring = self._fields()
        if it == 0:
            raise ValueError("the meter has seen no batch")
        f1, rec, prec, idx = ring[(it - 1) % self.window].tolist()
        return float(f1), float(rec), float(prec), self.thresholds[int(idx)]

    def window_median(self):
        """f1 / recall / precision medians over the last min(window, n) batches and the last batch's threshold
        (ScalarMeter.get_win_median and the ``threshold`` field of log_iter_stats, meters.py:181-185,305-308)."""
        it, _, _, _, ring = self._fields()
        if it == 0:
            raise ValueError("the meter has seen no batch")
        rows = ring[:min(it, self.window)].astype(np.float64)      # the median does not depend on the order inside the ring
        return {"f1": float(np.median(rows[:, 0])), "recall": float(np.median(rows[:, 1])),
                "precision": float(np.median(rows[:, 2])),
                "threshold": float(self.thresholds[int(ring[(it - 1) % self.window, 3])])}

    def epoch_stats(self):
        """log_epoch_stats (meters.py:332-334,468-470): recall = total / samples, precision likewise, f1 from the two.  With
        zero samples the reference raises ZeroDivisionError; here the three values are NaN."""
        _, _, tot, _, _ = self._fields()
        n = float(tot[2])
        recall = float(tot[0]) / n if n else float("nan")
        precision = float(tot[1]) / n if n else float("nan")
        return {"f1": 2 * recall * precision / (recall + precision + 1e-6), "recall": recall, "precision": precision, "samples": n}

    def dataset_stats(self):
        """TestGazeMeter.finalize_metrics (meters.py:132-146): ONE adaptive F1 over every frame seen, with one common best
        threshold, from the per-threshold sums instead of the kept predictions."""
        _, frames, _, sums, _ = self._fields()
        if frames == 0:
            nan = float("nan")
            return {"f1": nan, "recall": nan, "precision": nan, "threshold": float(self.thresholds[0]), "frames": 0}
        recall, precision = sums[0] / frames, sums[1] / frames
        f1 = 2 * recall * precision / (recall + precision + 1e-6)
        i = int(np.argmax(f1))
        return {"f1": float(f1[i]), "recall": float(recall[i]), "precision": float(precision[i]),
                "threshold": float(self.thresholds[i]), "frames": frames}


def _meter_setup(self, dataset, window, mode):
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {_MODES}, got {mode!r}")
    if int(window) < 1:
        raise ValueError("window must be >= 1")
    self.dataset, self.window, self.mode = dataset, int(window), mode
    self.fixation = fixation_index(dataset)
    self.thresholds = thresholds_for(dataset)
    self.lib = L.load()
    self.state_bytes = int(self.lib.csts_gaze_meter_state_bytes(len(self.thresholds), self.window))
    assert self.state_bytes % 8 == 0 and self.state_bytes > 0


class HostGazeMeter(_MeterReader):
    """The meter on host memory through csts_gaze_meter_update_host: the arithmetic of the device kernel without a GPU.
    It is fed per-frame counts (the layout f1_count_kernel writes), not heat maps."""

    def __init__(self, dataset, window, mode="train"):
        _meter_setup(self, dataset, window, mode)
        self.state = np.zeros(self.state_bytes // 8, dtype=np.int64)

    def _state_host(self):
        return self.state

    def reset(self):
        self.state[:] = 0

    def update_counts(self, counts, labels, batch_size=None):
        """counts (nframes, 2 nthr + 1) int32, labels (..., L >= 3) float64 with the gaze type in [..., 2]; ``batch_size`` is
        the train meter's mb_size (clips of the gathered batch)."""
        n = len(self.thresholds)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.float64).reshape(-1, np.shape(labels)[-1]))
        assert counts.shape == (lab.shape[0], 2 * n + 1) and lab.shape[1] >= 3, (counts.shape, lab.shape)
        if self.mode == "train" and batch_size is None:
            raise ValueError("a train meter needs the batch size")
        mb = int(batch_size) if self.mode == "train" else -1
        L.check(self.lib.csts_gaze_meter_update_host(counts.ctypes.data, lab.ctypes.data + 16, lab.shape[1], lab.shape[0], n,
                                                     self.fixation, _WEIGHT_TYPE, mb, self.window, self.state.ctypes.data),
                "csts_gaze_meter_update_host")


class GazeMeter(_MeterReader):
    """TrainGazeMeter / ValGazeMeter / TestGazeMeter (slowfast/utils/meters.py) as device-resident running statistics.

    ``update`` launches the count kernel and the one-workgroup update kernel (csts_f1_counts, csts_gaze_meter_update) on the
    current stream and never synchronises, allocates nothing after its first call at a given batch shape and reads nothing
    on the host, so it can be captured into a HIP graph; the iteration counter lives in the state buffer.  Between ranks the
    per-frame integer counts and the labels are all-gathered (the metric of the gathered batch depends on nothing else),
    not the predictions.  ``window_median`` / ``epoch_stats`` / ``dataset_stats`` / ``last_batch`` copy the state to the host.

    mode "train": a batch weighs its number of clips over all ranks (meters.py:272-280).  "val" / "test": a batch weighs its
    number of frames with gaze type 1 (meters.py:87-88,409-410), followed literally although the tracked type is 0."""

    def __init__(self, dataset, window, device, mode="train"):
        _meter_setup(self, dataset, window, mode)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.CstsError("csts_amd.metrics.GazeMeter runs on MI355X only (HostGazeMeter is the host twin)")
        self.state = torch.zeros(self.state_bytes // 8, dtype=torch.int64, device=self.device)
        self.thr_d = torch.tensor(self.thresholds.astype(np.float32), device=self.device)
        self._counts, self._labels = {}, {}

    def _state_host(self):
        return self.state.cpu().numpy()

    def reset(self):
        L.check(self.lib.csts_gaze_meter_reset(self.state.data_ptr(), len(self.thresholds), self.window,
                                               torch.cuda.current_stream().cuda_stream), "csts_gaze_meter_reset")

    def _buffer(self, key, nframes):
        buf = self._counts.get((key, nframes))
        if buf is None:
            buf = self._counts[(key, nframes)] = torch.empty(nframes, 2 * len(self.thresholds) + 1, dtype=torch.int32,
                                                             device=self.device)
        return buf

    def update(self, preds, labels_hm, labels, rescale: bool = True, world=None):
        """preds (B, 1, T, H, W) heat maps of THIS rank (softmaxed; min-max rescaled here unless rescale=False), labels_hm
        (B, T, H, W), labels (B, T, L >= 3).  world=None: the size of the default process group if one is up, else 1."""
        n = len(self.thresholds)
        p = preds.detach().squeeze(1).contiguous().float()
        q = labels_hm.detach().contiguous().float()
        B, T, H, W = q.shape
        assert p.shape == q.shape, (p.shape, q.shape)
        lab = labels.detach().reshape(B * T, -1).contiguous().double()
        assert lab.shape[1] >= 3, lab.shape
        if world is None:
            from . import distributed as du
            world = torch.distributed.get_world_size() if du.is_dist() else 1
        stream = torch.cuda.current_stream().cuda_stream
        counts = self._buffer("local", B * T)
        L.check(self.lib.csts_f1_counts(p.data_ptr(), q.data_ptr(), self.thr_d.data_ptr(), n, B * T, H * W, 1 if rescale else 0,
                                        counts.data_ptr(), stream), "csts_f1_counts")
        if world != 1:
            # the metric of the gathered batch (train_avgaze_net.py:114,194) depends on these integers and the labels only
            allc = self._buffer("gathered", world * B * T)
            alll = self._labels.get((world * B * T, lab.shape[1]))
            if alll is None:
                alll = self._labels[(world * B * T, lab.shape[1])] = torch.empty(world * B * T, lab.shape[1], dtype=torch.float64,
                                                                                 device=self.device)
            torch.distributed.all_gather(list(allc.chunk(world)), counts)
            torch.distributed.all_gather(list(alll.chunk(world)), lab)
            counts, lab = allc, alll
        mb = B * world if self.mode == "train" else -1
        L.check(self.lib.csts_gaze_meter_update(counts.data_ptr(), lab.data_ptr() + 16, lab.shape[1], lab.shape[0], n, self.fixation,
                                                _WEIGHT_TYPE, mb, self.window, self.state.data_ptr(), stream),
                "csts_gaze_meter_update")
