"""ROS1 optical-flow node (reference ros/scripts/main.py:25-160).

Topics / parameters are those of the reference so existing launch files work:

* subscribes ``rosparam /ROS/prev_img`` and ``/ROS/curr_img`` (sensor_msgs/Image);
* publishes the colour-coded flow on ``/raft_result`` (queue_size 100), encoding
  ``passthrough`` (BGR uint8), header = the *current* image's header with
  ``frame_id = "raft_image"``;
* ``/RAFT/weight_path``, ``/RAFT/is_small``, ``/RAFT/device``; 20 refinement
  iterations unless ``/RAFT/iters``, fp32 (``mixed_precision = False``) unless
  ``/RAFT/mixed_precision``;
* ``/RAFT/warm_start`` (default off): a pair whose previous frame is the last pair's current
  frame (equal stamps, same size) starts from that pair's flow, forward-projected on the
  device (``ops/warm_start.py``);
* ``/RAFT/device_io`` (default off): on a GPU device the frames are uploaded as they arrive
  (uint8, HWC; a quarter of the fp32 upload) and converted and padded by one HIP launch, and
  the flow is colour-coded on the device, so that only the uint8 image comes back
  (``ops/frame_io.py``).  The flow is bitwise the same; the image may differ from the numpy
  colour coding by one level on rare pixels.  On a CPU device the parameter changes nothing.
* ``/RAFT/occlusion`` (default off): the flow is computed in both directions (one batch of the
  pair and the swapped pair) and checked forward against backward (``ops/consistency.py``); the
  mask is published on ``/raft_occlusion`` (queue_size 100), encoding ``mono8``, with the header
  of the result: 0 = consistent, 128 = inconsistent (occluded or mismatched), 255 = the flow
  leaves the frame.  With the parameter off there is no second publisher.
* ``/RAFT/track`` (default off) and ``/RAFT/track_cell`` (default 32): a grid of points, one per
  cell of the image, is followed through the flow on the device (``ops/track.py``) and published
  on ``/raft_tracks`` (queue_size 100) as ``sensor_msgs/PointCloud`` with the header of the result:
  the tracked points ``(x, y, 0)`` in image coordinates with the channels ``id`` (``id mod 2^24``),
  ``prev_x``, ``prev_y`` and ``age``.  Pairs are continuous by warm start's stamp rule; with
  ``/RAFT/occlusion`` the forward-backward check drops inconsistent points.  With the parameter
  off there is no third publisher.
* ``/RAFT/track_seeds`` (default ``grid``): where a new point starts.  ``grid`` is the centre of
  its cell; ``corners`` is the cell's Shi-Tomasi corner, found on the device from the uint8 frames
  (``ops/corners.py``), and ``/raft_tracks`` gets a further channel ``score``, the corner score each
  point was born with.  ``/RAFT/track_min_score`` (default 0): cells whose best score is not above
  it keep their centre.
* ``/RAFT/scale`` (default 1): the working resolution.  With an integer ``D`` in 2..8 the model runs
  on the frames reduced by ``D`` (box filter, ``ops/frame_scale.py``) and its flow is brought back
  to the camera's resolution and pixel units (bilinear, times ``D``) before anything else reads
  it: the published image, the mask and the track coordinates are those of the unpadded camera
  frame ``H x W``.  With 1 nothing changes.

Pairing rule (reference :87-114): take the oldest current frame, then discard
previous frames until one with a stamp strictly earlier than the current one is
found; pair those.  Differences, all behavioural fixes:

* the worker blocks on a condition variable instead of busy-spinning;
* ``torch.load`` uses ``map_location`` (CPU-saved or GPU-saved weights work on
  either), no DataParallel wrapper is needed to strip ``module.``;
* the model runs through the HIP kernels on MI355X (``/RAFT/device: cuda``).

The ROS-independent part (``FramePairer`` and ``FlowInference``) is importable
without rospy; ``RaftRosNode`` needs rospy, sensor_msgs and cv_bridge.
"""
from __future__ import annotations

import collections
import threading
from argparse import Namespace
from typing import Any, Callable, Optional, Tuple

import numpy as np
import torch

from ..models import RAFT
from ..ops.consistency import OCC_LEVELS, fb_consistency
from ..ops.corners import corner_seeds, slot_scores
from ..ops.frame_io import flow_to_image, ingest_frames
from ..ops.frame_scale import ingest_frames_scaled, scaled_shape, upscale_flow
from ..ops.track import PointTracker
from ..ops.warm_start import forward_splat_nearest
from ..runtime import GraphedRAFT
from ..utils import checkpoint, flow_viz
from ..utils.utils import InputPadder


def _stamp_sec(msg) -> float:
    st = msg.header.stamp
    return st.to_sec() if hasattr(st, "to_sec") else float(st)


class FramePairer:
    """Thread-safe prev/curr frame queues with the reference's pairing rule."""

    def __init__(self):
        self._prev = collections.deque()
        self._curr = collections.deque()
        self._cv = threading.Condition()
        self._closed = False

    def push_prev(self, msg) -> None:
        with self._cv:
            self._prev.append(msg)
            self._cv.notify()

    def push_curr(self, msg) -> None:
        with self._cv:
            self._curr.append(msg)
            self._cv.notify()

    def close(self) -> None:
        with self._cv:
            self._closed = True
            self._cv.notify_all()

    def try_pair(self) -> Optional[Tuple[Any, Any]]:
        """Pop one (prev, curr) pair if available (caller holds no lock)."""
        with self._cv:
            return self._pair_locked()

    def _pair_locked(self):
        if not self._curr or not self._prev:
            return None
        curr = self._curr.popleft()
        while self._prev:
            prev = self._prev.popleft()
            if _stamp_sec(prev) < _stamp_sec(curr):
                return prev, curr
        return None  # no earlier prev frame: the current frame is dropped (as in the reference)

    def wait_pair(self, timeout: Optional[float] = None):
        with self._cv:
            while not self._closed:
                pair = self._pair_locked()
                if pair is not None:
                    return pair
                if not self._cv.wait(timeout):
                    return None
            return None


class FlowInference:
    """RAFT inference on numpy HxWx3 uint8 frames -> BGR uint8 flow visualisation.

    ``scale = D`` in 2..8 sets a working resolution: the model runs on the frames reduced by ``D``
    (``ops/frame_scale.py``) and every public method passes its flow through ``upscale_flow`` once,
    so that flows, images, masks and tracks are those of the *unpadded* camera frame ``H x W``
    (not of the padded frame, as with ``scale = 1``), in the camera's pixel units.  Warm start
    keeps working on the low-resolution flow."""

    def __init__(self, weight_path: Optional[str], small: bool = False, device: str = "cuda", iters: int = 20,
                 mixed_precision: bool = False, hip_graph: bool = True, warm_start: bool = False,
                 device_io: bool = False, consistency: bool = False, track: bool = False, track_cell: int = 32,
                 scale: int = 1, track_seeds: str = "grid", track_min_score: int = 0):
        if track_seeds not in ("grid", "corners"):
            raise ValueError(f"FlowInference: track_seeds is 'grid' or 'corners', got {track_seeds!r}")
        if isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= 8:
            raise ValueError(f"FlowInference: expected an integer scale in 1..8, got {scale!r}")
        self.scale = scale
        if device.startswith("cuda") and not torch.cuda.is_available():
            device = "cpu"
        self.device = torch.device(device)
        self.iters = iters
        self.args = Namespace(small=small, mixed_precision=mixed_precision, alternate_corr=False)
        self.model = RAFT(self.args)
        if weight_path:
            checkpoint.load_weights(self.model, weight_path, map_location="cpu")
        self.model.to(self.device).eval()
        # camera streams have a fixed frame size: capture the forward once, replay per pair
        self.runner = GraphedRAFT(self.model, iters=iters, enabled=hip_graph)
        # warm start (video): the last pair's low-resolution flow, forward-projected onto its
        # current frame, initialises the next pair when that pair starts at the same frame
        self.warm_start = warm_start
        self.reset_warm_start()
        # device-side frame path (GPU only): uint8 upload + HIP ingest, HIP colour coding; the
        # pinned staging buffers are kept while the frame size stays the same
        self.device_io = device_io
        self._pin_in: Optional[torch.Tensor] = None
        self._pin_in_free: Optional[torch.cuda.Event] = None
        self._pin_out: Optional[torch.Tensor] = None
        # bidirectional mode (flow_checked / visualize_checked): the pair and the swapped pair as
        # one batch of two, then the forward-backward check of ops/consistency.py
        self.consistency = consistency
        self.last_counts: Optional[np.ndarray] = None  # pixels of class 1 / 2 of the last visualize_checked
        self._pin_occ: Optional[torch.Tensor] = None
        self._pin_counts: Optional[torch.Tensor] = None
        # point tracks (tracks / visualize_tracks): a grid of points, one per track_cell x track_cell
        # cell of the unpadded image, kept on the device and advanced by every pair's flow
        # (ops/track.py); continuous pairs are recognised by warm start's stamp rule
        self.track = track
        self.track_cell = int(track_cell)
        self._tracker = PointTracker(S=self.track_cell) if track else None
        self._track_stamp = None
        self._track_shape = None
        self._track_shift = None  # (roi, the fp32 (left, top) on the device)
        self._pins = {}  # pinned return buffers of the tracks, by name
        # where a new point starts: "grid", the centre of its cell, or "corners", the cell's
        # Shi-Tomasi corner in the uint8 camera frame (ops/corners.py); with corners a sixth array,
        # the score each point was born with, is kept next to the tracker's state
        self.track_seeds = track_seeds
        self.track_min_score = int(track_min_score)
        self._frames_u8: Optional[torch.Tensor] = None  # the uint8 pair of the last upload, on the device
        self._track_score: Optional[torch.Tensor] = None

    def reset_warm_start(self) -> None:
        """Forget the previous pair: the next call runs cold."""
        self._warm_flow: Optional[torch.Tensor] = None
        self._warm_stamp = None
        self._warm_shape = None

    @property
    def _on_device(self) -> bool:
        return self.device_io and self.device.type == "cuda"

    def _ingest(self, prev: np.ndarray, curr: np.ndarray):
        """The pair as uint8 through one pinned buffer -> the padded fp32 images on the device."""
        a = torch.from_numpy(np.ascontiguousarray(prev, dtype=np.uint8))
        b = torch.from_numpy(np.ascontiguousarray(curr, dtype=np.uint8))
        if a.shape != b.shape or a.dim() != 3:
            raise ValueError(f"frames must be two (H, W, 3) images of one size, got {tuple(a.shape)}, {tuple(b.shape)}")
        if self._pin_in is None or self._pin_in.shape[1:] != a.shape:
            self._pin_in = torch.empty((2,) + tuple(a.shape), dtype=torch.uint8, pin_memory=True)
            self._pin_in_free = torch.cuda.Event()
        else:
            self._pin_in_free.synchronize()  # the last pair's upload has read the buffer
        self._pin_in[0].copy_(a)
        self._pin_in[1].copy_(b)
        with torch.cuda.device(self.device):
            frames = self._pin_in.to(self.device, non_blocking=True)
            self._pin_in_free.record()
        self._frames_u8 = frames
        images, _ = ingest_frames(frames) if self.scale == 1 else ingest_frames_scaled(frames, self.scale)
        return images[0:1], images[1:2]

    def _padded_pair(self, prev: np.ndarray, curr: np.ndarray):
        """The two frames as the model takes them: (1, 3, Hp, Wp) fp32 on the device, padded; with
        ``scale > 1`` reduced to the working resolution first."""
        if self._on_device:
            return self._ingest(prev, curr)
        if self.scale > 1:  # a plain uint8 upload, then the downscale where the model runs
            frames = torch.stack([torch.from_numpy(np.ascontiguousarray(prev, dtype=np.uint8)),
                                  torch.from_numpy(np.ascontiguousarray(curr, dtype=np.uint8))]).to(self.device)
            self._frames_u8 = frames
            images, _ = ingest_frames_scaled(frames, self.scale)
            return images[0:1], images[1:2]
        image1 = torch.from_numpy(np.ascontiguousarray(prev, dtype=np.uint8)).permute(2, 0, 1).float()[None]
        image2 = torch.from_numpy(np.ascontiguousarray(curr, dtype=np.uint8)).permute(2, 0, 1).float()[None]
        image1, image2 = image1.to(self.device), image2.to(self.device)
        padder = InputPadder(image1.shape)
        return padder.pad(image1, image2)

    def _run(self, image1, image2, prev_stamp, curr_stamp, both: bool = False) -> torch.Tensor:
        """flow_up of the padded pair, or with ``both`` of the batch [pair, swapped pair].  With
        ``warm_start`` the call is warm only when ``prev_stamp`` is given and equals the last call's
        ``curr_stamp`` and the padded shape is unchanged; any other call runs cold and drops the
        kept state.  The kept state is the forward direction's alone."""
        shape = tuple(image1.shape)
        if both:
            image1, image2 = torch.cat([image1, image2]), torch.cat([image2, image1])
        if not self.warm_start:
            _, flow_up = self.runner(image1, image2)
            return flow_up
        warm = (self._warm_flow is not None and prev_stamp is not None and prev_stamp == self._warm_stamp
                and shape == self._warm_shape)
        flow_init = self._warm_flow if warm else None
        self.reset_warm_start()
        if flow_init is None:
            flow_low, flow_up = self.runner(image1, image2)
        else:
            if both:  # the backward direction has no previous flow: it always starts cold
                flow_init = torch.cat([flow_init, torch.zeros_like(flow_init)])
            flow_low, flow_up = self.runner(image1, image2, flow_init=flow_init)
        if curr_stamp is not None:
            # flow_low may be a captured graph's static output, overwritten by the next replay:
            # the splat reads it now and writes a fresh tensor
            self._warm_flow = forward_splat_nearest(flow_low[0:1])
            self._warm_stamp, self._warm_shape = curr_stamp, shape
        return flow_up

    def _upscale(self, flow_up: torch.Tensor, frame: np.ndarray) -> torch.Tensor:
        """``scale > 1``: the model's flow on the padded low-resolution frame -> the flow of the
        unpadded camera frame (B, 2, H, W).  ``flow_up`` may be a captured graph's static output: the
        op reads it now and writes a fresh tensor."""
        H, W = frame.shape[:2]
        return upscale_flow(flow_up, InputPadder(scaled_shape(H, W, self.scale)), self.scale, (H, W))

    @torch.inference_mode()
    def flow(self, prev: np.ndarray, curr: np.ndarray, prev_stamp=None, curr_stamp=None) -> torch.Tensor:
        """Flow of the padded pair.  With ``warm_start`` the call is warm only when ``prev_stamp``
        is given and equals the last call's ``curr_stamp`` and the padded shape is unchanged;
        any other call runs cold and drops the kept state.  With ``scale > 1`` the result is the flow
        of the unpadded camera frame, (1, 2, H, W)."""
        flow_up = self._run(*self._padded_pair(prev, curr), prev_stamp, curr_stamp)
        return flow_up if self.scale == 1 else self._upscale(flow_up, prev)

    @torch.inference_mode()
    def flow_checked(self, prev: np.ndarray, curr: np.ndarray, prev_stamp=None, curr_stamp=None):
        """Bidirectional mode: (flow_fw, occ, err2, counts) of the padded pair.

        The model runs once on the batch of the pair and the swapped pair; image 0 of its output is
        the forward flow (what ``flow()`` computes), image 1 the backward flow, and
        ``ops.consistency.fb_consistency`` checks one against the other.  With ``warm_start`` the
        pairing rule is ``flow()``'s; only the forward direction is kept and only it starts warm.  With ``scale > 1`` both
        directions are upscaled in one call and everything is of the unpadded camera frame."""
        if not self.consistency:
            raise RuntimeError("flow_checked needs FlowInference(consistency=True)")
        flow_up = self._run(*self._padded_pair(prev, curr), prev_stamp, curr_stamp, both=True)
        if self.scale > 1:
            flow_up = self._upscale(flow_up, prev)
        flow_fw = flow_up[0:1]
        occ, err2, counts = fb_consistency(flow_fw, flow_up[1:2])
        return flow_fw, occ, err2, counts

    def visualize_checked(self, prev: np.ndarray, curr: np.ndarray, prev_stamp=None, curr_stamp=None):
        """(the image ``visualize`` returns, the mask as mono uint8 (H, W): 0 consistent, 128
        inconsistent, 255 the flow leaves the frame; ``H x W`` of the camera frame with ``scale > 1``).  The counts of the two classes are kept as
        ``last_counts``.  With ``device_io`` everything comes back through pinned buffers under
        one synchronisation."""
        if self._on_device:
            with torch.inference_mode():
                flow_fw, occ, _, counts = self.flow_checked(prev, curr, prev_stamp, curr_stamp)
                img = flow_to_image(flow_fw, convert_to_bgr=True)[0]
                if self._pin_out is None or self._pin_out.shape != img.shape:
                    self._pin_out = torch.empty(tuple(img.shape), dtype=torch.uint8, pin_memory=True)
                if self._pin_occ is None or self._pin_occ.shape != occ.shape[1:]:
                    self._pin_occ = torch.empty(tuple(occ.shape[1:]), dtype=torch.uint8, pin_memory=True)
                    self._pin_counts = torch.empty((2,), dtype=torch.int32, pin_memory=True)
                self._pin_out.copy_(img, non_blocking=True)
                self._pin_occ.copy_(occ[0], non_blocking=True)
                self._pin_counts.copy_(counts[0], non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
            self.last_counts = self._pin_counts.numpy().copy()
            # the buffers are reused: the caller gets its own memory (the level look-up writes a new array)
            return self._pin_out.numpy().copy(), OCC_LEVELS[self._pin_occ.numpy()]
        flow_fw, occ, _, counts = self.flow_checked(prev, curr, prev_stamp, curr_stamp)
        rgb = flow_viz.flow_to_image(flow_fw[0].permute(1, 2, 0).float().cpu().numpy())
        self.last_counts = counts[0].cpu().numpy().copy()
        return np.ascontiguousarray(rgb[:, :, [2, 1, 0]]).astype(np.uint8), OCC_LEVELS[occ[0].cpu().numpy()]

    def visualize(self, prev: np.ndarray, curr: np.ndarray, prev_stamp=None, curr_stamp=None) -> np.ndarray:
        """The published image: colour-coded flow of the *padded* pair, BGR uint8
        (reference convert2Img + inferRAFT, ros/scripts/main.py:70-80,117-149).  With ``scale > 1``
        the image is the unpadded camera frame's, ``H x W``, not the padded size."""
        if self._on_device:
            with torch.inference_mode():
                img = flow_to_image(self.flow(prev, curr, prev_stamp, curr_stamp), convert_to_bgr=True)[0]
                if self._pin_out is None or self._pin_out.shape != img.shape:
                    self._pin_out = torch.empty(tuple(img.shape), dtype=torch.uint8, pin_memory=True)
                self._pin_out.copy_(img, non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
            return self._pin_out.numpy().copy()  # the buffer is reused: the caller gets its own memory
        flo = self.flow(prev, curr, prev_stamp, curr_stamp)[0].permute(1, 2, 0).float().cpu().numpy()
        rgb = flow_viz.flow_to_image(flo)
        return np.ascontiguousarray(rgb[:, :, [2, 1, 0]]).astype(np.uint8)

    # ------------------------------------------------------------------ point tracks
    def _tracks_device(self, prev: np.ndarray, curr: np.ndarray, prev_stamp, curr_stamp):
        """One model run and one tracker step -> (flow_up of the run, the step's arrays in image
        coordinates as device tensors).  The pair continues the last one when ``prev_stamp`` is
        given and equals the last call's ``curr_stamp`` and the padded shape is unchanged (warm
        start's rule); any other pair seeds the grid anew.  With ``scale > 1`` the flow is the
        upscaled one and the points live on the whole camera frame: no pad shift."""
        if not self.track:
            raise RuntimeError("tracks needs FlowInference(track=True)")
        h, w = prev.shape[:2]
        self._frames_u8 = None
        image1, image2 = self._padded_pair(prev, curr)
        shape = tuple(image1.shape)
        if self.scale > 1:
            shape += (h, w, self.scale)  # one low-resolution shape serves several camera sizes
        continuous = prev_stamp is not None and prev_stamp == self._track_stamp and shape == self._track_shape
        flow_up = self._run(image1, image2, prev_stamp, curr_stamp, both=self.consistency)
        if self.scale > 1:
            flow_up = self._upscale(flow_up, prev)
            roi = (0, 0, w, h)  # the camera frame itself
        else:
            pad = InputPadder((h, w))._pad
            roi = (pad[0], pad[2], w, h)  # the unpadded image inside the padded frame
        fw = flow_up[0:1].float().contiguous()
        bw = flow_up[1:2].float().contiguous() if self.consistency else None
        seeds = {}
        if self.track_seeds == "corners":
            frames = self._frames_u8
            if frames is None:  # the pair went up as fp32: one more upload, as uint8
                frames = torch.stack([torch.from_numpy(np.ascontiguousarray(prev, dtype=np.uint8)),
                                      torch.from_numpy(np.ascontiguousarray(curr, dtype=np.uint8))]).to(self.device)
            self._frames_u8 = None
            # image 0 serves a (re)seeded grid, whose points start in the first frame; image 1 the
            # points born in this step, which live in the second
            corners, cell_score = corner_seeds(frames, self.track_cell, (w, h), roi[:2],
                                               min_score=self.track_min_score)
            seeds = dict(first_seeds=corners[0:1], seeds=corners[1:2])
        resets = self._tracker.resets
        pos, prv, ids, age, _, status, _, _ = self._tracker.update(fw, bw, continuous=continuous, roi=roi, **seeds)
        self._track_stamp, self._track_shape = curr_stamp, shape
        if self._track_shift is None or self._track_shift[0] != (roi, fw.device):
            self._track_shift = ((roi, fw.device), torch.tensor([roi[0], roi[1]], dtype=torch.float32).to(fw.device))
        shift = self._track_shift[1]
        arrays = dict(points=(pos - shift)[0], prev=(prv - shift)[0], ids=ids[0], age=age[0], status=status[0])
        if seeds:
            kept = None
            if self._tracker.resets == resets:  # the pair continued: the survivors keep their score
                kept = self._track_score
            else:  # a fresh grid: slot j was born on the first frame's seed of cell j
                kept = cell_score[0:1]
            self._track_score = slot_scores(pos, age, kept, cell_score[1:2], roi, self.track_cell)
            arrays["score"] = self._track_score[0]
        return flow_up, arrays

    def _to_pinned(self, name: str, t: torch.Tensor) -> torch.Tensor:
        pin = self._pins.get(name)
        if pin is None or pin.shape != t.shape or pin.dtype != t.dtype:
            pin = self._pins[name] = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
        pin.copy_(t, non_blocking=True)
        return pin

    def tracks(self, prev: np.ndarray, curr: np.ndarray, prev_stamp=None, curr_stamp=None):
        """(flow of the padded pair -- with ``scale > 1`` of the unpadded camera frame --, the point
        tracks of the unpadded image).

        The tracks are numpy arrays over the N slots of the grid, in image coordinates (frame
        coordinates minus the left / top pad): ``points`` (N, 2) fp32 (x, y) in the current frame,
        ``prev`` (N, 2) where each was in the previous frame (NaN for a new point), ``ids`` (N,)
        int64, ``age`` (N,) int32 and ``status`` (N,) uint8, the fate of the point the slot held
        before: 0 tracked (the only slots whose ``prev`` is a correspondence), 1 inconsistent, 2 left
        the image, 3 crowded out.  With ``track_seeds="corners"`` a sixth array ``score`` (N,) int32:
        the corner score the slot's point was born with (-1: a cell without candidates).  With ``consistency`` the model runs on the pair and the swapped
        pair and the forward-backward check applies; otherwise only the frame test.  With
        ``device_io`` the arrays come back through pinned buffers under one synchronisation."""
        with torch.inference_mode():
            flow_up, arrays = self._tracks_device(prev, curr, prev_stamp, curr_stamp)
            if self._on_device:
                pins = {k: self._to_pinned(k, v) for k, v in arrays.items()}
                torch.cuda.current_stream(self.device).synchronize()
                return flow_up[0:1], {k: p.numpy().copy() for k, p in pins.items()}  # the buffers are reused
        return flow_up[0:1], {k: v.cpu().numpy().copy() for k, v in arrays.items()}

    def visualize_tracks(self, prev: np.ndarray, curr: np.ndarray, prev_stamp=None, curr_stamp=None):
        """(the image ``visualize`` returns, the mask of ``visualize_checked`` or None without
        ``consistency``, the tracks of ``tracks``) from one run of the model."""
        with torch.inference_mode():
            flow_up, arrays = self._tracks_device(prev, curr, prev_stamp, curr_stamp)
            flow_fw = flow_up[0:1]
            occ = counts = None
            if self.consistency:
                occ, _, counts = fb_consistency(flow_fw, flow_up[1:2])
            if self._on_device:
                pins = {k: self._to_pinned(k, v) for k, v in arrays.items()}
                img = self._to_pinned("image", flow_to_image(flow_fw, convert_to_bgr=True)[0])
                if occ is not None:
                    occ, counts = self._to_pinned("occ", occ[0]), self._to_pinned("counts", counts[0])
                torch.cuda.current_stream(self.device).synchronize()
                if occ is not None:
                    self.last_counts = counts.numpy().copy()
                return (img.numpy().copy(), None if occ is None else OCC_LEVELS[occ.numpy()],
                        {k: p.numpy().copy() for k, p in pins.items()})
        rgb = flow_viz.flow_to_image(flow_fw[0].permute(1, 2, 0).float().cpu().numpy())
        if occ is not None:
            self.last_counts = counts[0].cpu().numpy().copy()
        return (np.ascontiguousarray(rgb[:, :, [2, 1, 0]]).astype(np.uint8),
                None if occ is None else OCC_LEVELS[occ[0].cpu().numpy()],
                {k: v.cpu().numpy().copy() for k, v in arrays.items()})


class RaftRosNode:
    """The ROS node; all ROS modules are injected at construction for testability."""

    def __init__(self, rospy=None, image_msg=None, cv_bridge_cls=None, inference: Optional[FlowInference] = None,
                 track_msgs=None):
        """``track_msgs``: the message classes (PointCloud, Point32, ChannelFloat32) of
        ``/raft_tracks``; imported from sensor_msgs / geometry_msgs when ``/RAFT/track`` is set and
        none are given."""
        if rospy is None:
            import rospy  # noqa: F811
        if image_msg is None:
            from sensor_msgs.msg import Image as image_msg  # noqa: F811
        if cv_bridge_cls is None:
            from cv_bridge import CvBridge as cv_bridge_cls  # noqa: F811
        self.rospy = rospy
        self.bridge = cv_bridge_cls()
        rospy.init_node("raft_ros", anonymous=True)
        self.pairer = FramePairer()
        rospy.Subscriber(rospy.get_param("/ROS/prev_img"), image_msg, self.callbackPrevImage)
        rospy.Subscriber(rospy.get_param("/ROS/curr_img"), image_msg, self.callbackCurrImage)
        self._pub = rospy.Publisher("/raft_result", image_msg, queue_size=100)
        self.warm_start = bool(_get_param(rospy, "/RAFT/warm_start", False))
        self.occlusion = bool(_get_param(rospy, "/RAFT/occlusion", False))
        self._pub_occ = rospy.Publisher("/raft_occlusion", image_msg, queue_size=100) if self.occlusion else None
        self.track = bool(_get_param(rospy, "/RAFT/track", False))
        self.track_cell = int(_get_param(rospy, "/RAFT/track_cell", 32))
        self.track_seeds = str(_get_param(rospy, "/RAFT/track_seeds", "grid"))
        self.track_min_score = int(_get_param(rospy, "/RAFT/track_min_score", 0))
        self.scale = int(_get_param(rospy, "/RAFT/scale", 1))
        self._pub_tracks = None
        if self.track:
            if track_msgs is None:
                from geometry_msgs.msg import Point32
                from sensor_msgs.msg import ChannelFloat32, PointCloud

                track_msgs = (PointCloud, Point32, ChannelFloat32)
            self._track_msgs = track_msgs
            self._pub_tracks = rospy.Publisher("/raft_tracks", track_msgs[0], queue_size=100)
        if inference is None:
            print("Initialize RAFT...")
            inference = FlowInference(rospy.get_param("/RAFT/weight_path"), bool(rospy.get_param("/RAFT/is_small")),
                                      str(rospy.get_param("/RAFT/device")),
                                      iters=int(_get_param(rospy, "/RAFT/iters", 20)),
                                      mixed_precision=bool(_get_param(rospy, "/RAFT/mixed_precision", False)),
                                      hip_graph=bool(_get_param(rospy, "/RAFT/hip_graph", True)),
                                      warm_start=self.warm_start,
                                      device_io=bool(_get_param(rospy, "/RAFT/device_io", False)),
                                      consistency=self.occlusion,
                                      **(dict(scale=self.scale) if self.scale != 1 else {}),
                                      **(dict(track=True, track_cell=self.track_cell) if self.track else {}),
                                      **(dict(track_seeds=self.track_seeds, track_min_score=self.track_min_score)
                                         if self.track and self.track_seeds != "grid" else {}))
            print("Initialize RAFT finish!")
        self.inference = inference
        self._thread: Optional[threading.Thread] = None

    # reference callback names
    def callbackPrevImage(self, msg) -> None:
        self.pairer.push_prev(msg)

    def callbackCurrImage(self, msg) -> None:
        self.pairer.push_curr(msg)

    def process_pair(self, prev_msg, curr_msg):
        prev = self.bridge.imgmsg_to_cv2(prev_msg, desired_encoding="passthrough")
        curr = self.bridge.imgmsg_to_cv2(curr_msg, desired_encoding="passthrough")
        # the message stamps tell the inference whether pairs are continuous
        stamps = (dict(prev_stamp=_stamp_sec(prev_msg), curr_stamp=_stamp_sec(curr_msg))
                  if self.warm_start or self.track else {})
        occ = tracks = None
        if self.track:
            result, occ, tracks = self.inference.visualize_tracks(np.asarray(prev), np.asarray(curr), **stamps)
        elif self.occlusion:
            result, occ = self.inference.visualize_checked(np.asarray(prev), np.asarray(curr), **stamps)
        else:
            result = self.inference.visualize(np.asarray(prev), np.asarray(curr), **stamps)
        header = curr_msg.header
        header.frame_id = "raft_image"
        out = self.bridge.cv2_to_imgmsg(result, encoding="passthrough", header=header)
        self._pub.publish(out)
        if occ is not None and self._pub_occ is not None:
            self._pub_occ.publish(self.bridge.cv2_to_imgmsg(occ, encoding="mono8", header=header))
        if tracks is not None:
            self._pub_tracks.publish(self.tracks_msg(tracks, header))
        return out

    def tracks_msg(self, tracks, header):
        """The tracked points (status 0) as a sensor_msgs/PointCloud: ``points[i] = (x, y, 0)`` in
        the current frame, channels ``id`` (``id mod 2^24``: exact in float32), ``prev_x``,
        ``prev_y`` (the same point in the previous frame) and ``age`` (pairs survived); with corner
        seeds also ``score``, the corner score the point was born with."""
        cloud_cls, point_cls, channel_cls = self._track_msgs
        keep = tracks["status"] == 0
        pts, prv = tracks["points"][keep], tracks["prev"][keep]
        msg = cloud_cls()
        msg.header = header
        msg.points = [point_cls(x=float(x), y=float(y), z=0.0) for x, y in pts]
        values = (("id", tracks["ids"][keep] % (1 << 24)), ("prev_x", prv[:, 0]), ("prev_y", prv[:, 1]),
                  ("age", tracks["age"][keep]))
        if "score" in tracks:
            values += (("score", tracks["score"][keep]),)
        msg.channels = [channel_cls(name=name, values=np.asarray(v, dtype=np.float32).tolist()) for name, v in values]
        return msg

    def thdInference(self, stop: Optional[Callable[[], bool]] = None) -> None:
        while not (stop and stop()) and not self.rospy.is_shutdown():
            pair = self.pairer.wait_pair(timeout=0.1)
            if pair is not None:
                self.process_pair(*pair)

    def start(self) -> threading.Thread:
        self._thread = threading.Thread(target=self.thdInference, daemon=True)
        self._thread.start()
        return self._thread

    def shutdown(self) -> None:
        self.pairer.close()


def _get_param(rospy, name, default):
    try:
        return rospy.get_param(name, default)
    except TypeError:  # minimal fakes without a default argument
        try:
            return rospy.get_param(name)
        except Exception:
            return default


def main():  # pragma: no cover - needs a ROS master
    import rospy

    node = RaftRosNode(rospy)
    node.start()
    rospy.spin()
    node.shutdown()
