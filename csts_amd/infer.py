"""Inference: trained weights in, gaze predictions out.

``GazePredictor`` is the public interface: it builds the model, loads a checkpoint by the reference's name-and-shape rule
(csts_amd.checkpoint) and turns uint8 frames + a waveform into a gaze point, its probability and the heat map of every frame,
all on the device.  What the reference's test driver does per batch (tools/test_avgaze_net.py:50-70: eval forward,
frame_softmax at temperature 2, per-frame min-max rescale) runs here as the model forward followed by ONE fused head kernel
(csts_gaze_decode), and ``GraphedEvalStep`` captures the two into one HIP graph: the forward is launch-bound from Python just
as the training step is, so replaying it is the eval counterpart of train.GraphedTrainStep."""
from __future__ import annotations

import torch

from . import checkpoint as ck
from . import lib as L
from . import ops

TEMPERATURE = 2.0          # frame_softmax temperature of the train / val / test drivers of the reference


def _core(model):
    return model.module if hasattr(model, "module") else model


def eval_forward(model, video, audio):
    """model([video], audio) -> gaze_decode, with the kernels the graph replays.  The caller holds eval mode and no_grad.
    Returns {"logits", "preds", "rescaled"}: (B, 1, T, H/4, W/4); "points": (B, T, 2); "peak": (B, T)."""
    logits = model([video], audio)
    out = ops.gaze_decode(logits, TEMPERATURE)
    out["logits"] = logits
    return out


class GraphedEvalStep:
    """The forward-only step -- eval-mode model([video], audio), then gaze_decode -- captured ONCE into a HIP graph and replayed.
    The capture runs the model's own forward, so the second-stream trunks of CSTS_AMD.TWO_STREAMS are part of the graph as
    they are in the training capture.  Inputs are copied into static buffers; run() returns the graph's static outputs, which
    the next run() overwrites.  The model's parameters are not touched and its training flag is put back."""

    def __init__(self, cfg, model, example_batch, warmup: int = 2):
        self.cfg, self.model = cfg, _core(model)      # forward only: nothing for a data-parallel wrapper to reduce
        for k in ("video", "audio"):
            if not example_batch[k].is_cuda:
                raise L.CstsError("GraphedEvalStep runs on MI355X only: the batch must hold GPU tensors")
        self.static = {k: example_batch[k].detach().clone() for k in ("video", "audio")}
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(max(1, warmup)):      # lazy tables, weight shadows and the allocator see the real thing
                        self._step()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                ops.refill_capture_pools()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                    self.out = self._step()
                torch.cuda.synchronize()
        finally:
            self.model.train(was_training)

    def _step(self):
        return eval_forward(self.model, self.static["video"], self.static["audio"])

    def run(self, video=None, audio=None):
        """Copy the inputs into the static buffers (None: keep what they hold) and replay.  Returns the static outputs
        {"logits", "preds", "rescaled", "points", "peak"}."""
        for k, v in (("video", video), ("audio", audio)):
            if v is not None and v is not self.static[k]:
                if v.shape != self.static[k].shape:
                    raise ValueError(f"{k} is {tuple(v.shape)}, this step was captured for {tuple(self.static[k].shape)}")
                self.static[k].copy_(v, non_blocking=True)
        if hasattr(self.model, "_refresh_w16"):
            was_training = self.model.training
            self.model.eval()
            try:
                with torch.no_grad():
                    self.model._refresh_w16()        # only acts after an out-of-band weight change (load_state_dict)
            finally:
                self.model.train(was_training)
        self.graph.replay()
        return self.out


class GazePredictor:
    """Gaze prediction with trained weights on one GPU.

    cfg: the model's configuration (NUM_GPUS 1).  checkpoint_path: a ``.pyth`` file, loaded by name and shape
    (checkpoint.load_checkpoint); None falls back to cfg.TEST.CHECKPOINT_FILE_PATH, and with that empty too the weights are the
    random initialisation (a warning says so).  graph=True replays one captured HIP graph per input shape (B, T, S);
    graph=False launches the same kernels eagerly -- the results are the same bit for bit."""

    def __init__(self, cfg, checkpoint_path=None, device=None, graph: bool = True):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise L.CstsError("GazePredictor runs on MI355X only: it needs a GPU device (there is no CPU fallback)")
        if cfg.NUM_GPUS != 1:
            raise ValueError(f"GazePredictor is one process on one GPU: build its cfg with NUM_GPUS 1, got {cfg.NUM_GPUS}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        from .build import build_model
        self.cfg, self.device, self.graph = cfg, device, bool(graph)
        with torch.cuda.device(device):
            self.model = build_model(cfg, gpu_id=device.index)
            if checkpoint_path is None:
                ck.load_test_checkpoint(cfg, self.model)
            else:
                ck.load_checkpoint(checkpoint_path, self.model)
        self.checkpoint_path = checkpoint_path if checkpoint_path is not None else (cfg.TEST.CHECKPOINT_FILE_PATH or None)
        self.model.eval()
        self._steps = {}           # (B, T, S) -> GraphedEvalStep

    @torch.no_grad()
    def predict(self, frames_u8, wav, frames_idx, frame_length, labels=None):
        """frames_u8 uint8 (B, T, H, W, 3), wav fp32 (B, n) at 24 kHz, frames_idx (B, T) = the sampled frames' positions on the
        clip's time axis of `frame_length` frames -> {"points": (B, T, 2) (x, y) in [0, 1), "peak": (B, T),
        "heatmaps": (B, T, S/4, S/4), "rescaled": same shape} on the device, S = DATA.TEST_CROP_SIZE.
        Frames that come at S x S are normalised as they are; any other size goes through the test-mode spatial sampling (short
        side to S, centre crop: inputs.spatial_sampling(train=False, spatial_idx=1)), so the points are in the crop's
        coordinates.  labels (optional, (B, T, L >= 2) gaze labels): carried through the same crop and returned as "labels"."""
        for t in (frames_u8, wav, frames_idx) + ((labels,) if labels is not None else ()):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise L.CstsError("GazePredictor runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
        from . import inputs
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 5 or frames_u8.shape[-1] != 3:
            raise ValueError(f"frames must be uint8 (B, T, H, W, 3), got {tuple(frames_u8.shape)} {frames_u8.dtype}")
        B, T, H, W, _ = frames_u8.shape
        if wav.dim() != 2 or wav.shape[0] != B or tuple(frames_idx.shape) != (B, T):
            raise ValueError(f"wav must be ({B}, n) and frames_idx ({B}, {T}), got {tuple(wav.shape)} and {tuple(frames_idx.shape)}")
        cfg = self.cfg
        S = int(cfg.DATA.TEST_CROP_SIZE)
        mean, std = tuple(cfg.DATA.MEAN), tuple(cfg.DATA.STD)
        with torch.cuda.device(self.device):
            new_labels = labels
            if (H, W) != (S, S):
                lab = labels if labels is not None else torch.zeros(B, T, 2, dtype=torch.float64, device=frames_u8.device)
                video, new_labels = inputs.spatial_sampling(frames_u8, lab, S, train=False, spatial_idx=1, mean=mean, std=std)
            else:
                video = inputs.normalize_frames(frames_u8, mean=mean, std=std)
            audio = inputs.audio_windows(inputs.stft_logpower(wav), frames_idx, frame_length)
            if S != 256:       # S frequency bins x S columns around each frame, as train.synthetic_batch cuts them
                o = (256 - S) // 2
                audio = audio[:, :, :, :S, o:o + S].contiguous()
            out = self.predict_batch({"video": video, "audio": audio})
        if labels is not None:
            out["labels"] = new_labels
        return out

    @torch.no_grad()
    def predict_batch(self, batch):
        """batch: an assembled dict with "video" fp32 (B, 3, T, S, S) and "audio" fp32 (B, 1, T, F, F) (inputs.assemble_batch,
        train.synthetic_batch) -> the dict of predict().  The tensors are the caller's: a later call does not overwrite them."""
        video, audio = batch["video"], batch["audio"]
        for t in (video, audio):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise L.CstsError("GazePredictor runs on MI355X only: inputs must be GPU tensors (there is no CPU fallback)")
        if video.dim() != 5 or audio.dim() != 5:
            raise ValueError(f"video and audio must be 5-D, got {tuple(video.shape)} and {tuple(audio.shape)}")
        with torch.cuda.device(self.device):
            if self.graph:
                key = (video.shape[0], video.shape[2], video.shape[-1])
                step = self._steps.get(key)
                if step is None or step.static["audio"].shape != audio.shape or step.static["video"].shape != video.shape:
                    step = self._steps[key] = GraphedEvalStep(self.cfg, self.model, {"video": video, "audio": audio})
                out = step.run(video, audio)
                out = {k: out[k].clone() for k in ("points", "peak", "preds", "rescaled")}
            else:
                out = eval_forward(self.model, video.contiguous(), audio.contiguous())
        return {"points": out["points"], "peak": out["peak"], "heatmaps": out["preds"].squeeze(1),
                "rescaled": out["rescaled"].squeeze(1)}
