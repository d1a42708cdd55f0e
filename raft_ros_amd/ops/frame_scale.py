"""Working-resolution inference: the model runs on frames reduced by an integer factor ``D`` and
its flow comes back at the camera's resolution and in the camera's pixel units.

* ``ingest_frames_scaled``: camera frames (uint8, HWC) -> the model's padded fp32 CHW input at
  ``ceil(H / D) x ceil(W / D)`` through ``raft_amd::ingest_frames_scaled`` (csrc/frame_scale.hip):
  the box (area) filter, cv2's ``INTER_AREA`` for integer factors, and the replicate padding in one
  launch.  Cell ``(i, j)`` covers rows ``[iD, min((i+1)D, H))`` and columns ``[jD, min((j+1)D, W))``;
  its value is ``float(sum) / float(count)`` with the integer sum of the cell's bytes and the
  number of its pixels inside the image (the last row / column of cells may be partial).
* ``upscale_flow``: the model's flow on the padded low-resolution frame -> the flow of the unpadded
  camera frame through ``raft_amd::upscale_flow``: bilinear with pixel centres aligned
  (``align_corners=False``), clamped at the border, times ``D``.  Per axis and output index ``x``
  over ``n`` low-resolution samples, in integers::

      q = x // D;  r = x % D;  t = 2r + 1 - D
      t >= 0:  i0 = q, num = t        else:  i0 = q - 1, num = t + 2D
      fx = float(num) / float(2D)     (one fp32 division; 0 when i0 < 0 or i0 >= n - 1)
      i0 = clamp(i0, 0, n - 1);  i1 = min(i0 + 1, n - 1)

  so a weight is one rounding of an exact rational at any width (the textbook
  ``(x + 0.5) / D - 0.5`` in fp32 loses bits as the width grows).  The value follows the lerp order
  of ``fb_consistency_ref``, one rounding a line::

      top = a01 - a00;  top = fx * top;  top = a00 + top
      bot = a11 - a10;  bot = fx * bot;  bot = a10 + bot
      s = bot - top;    s = fy * s;      s = top + s;      out = s * float(D)

* ``ingest_frames_scaled_ref`` / ``upscale_flow_ref``: the same arithmetic as plain torch ops, one
  op per rounding step, so that the HIP ops agree with them bitwise.  They are the CPU path and the
  tests' oracle.

Both ops are one launch on the current stream without host synchronisation.  ``D = 1`` is
``ingest_frames`` and ``InputPadder.unpad``.
"""
from __future__ import annotations

from typing import TYPE_CHECKING, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from ._ext import ops, use_native

if TYPE_CHECKING:  # utils.utils imports ops.reference: import it where it is used
    from ..utils.utils import InputPadder

MAX_SCALE = 8


def _check_scale(name: str, scale) -> int:
    if isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= MAX_SCALE:
        raise ValueError(f"{name}: expected an integer scale in 1..{MAX_SCALE}, got {scale!r}")
    return scale


def scaled_shape(H: int, W: int, D: int) -> Tuple[int, int]:
    """The low-resolution size ``(ceil(H / D), ceil(W / D))`` of an ``H x W`` frame."""
    D = _check_scale("scaled_shape", D)
    return -(-int(H) // D), -(-int(W) // D)


def ingest_frames_scaled_ref(frames: torch.Tensor, scale: int, pads: Sequence[int] = (0, 0, 0, 0)) -> torch.Tensor:
    """uint8 (N, H, W, 3) -> fp32 (N, 3, h + pad_t + pad_b, w + pad_l + pad_r), ``pads`` in
    ``F.pad`` order (left, right, top, bottom): integer cell sums, one fp32 division by the cell's
    pixel count, replicate padding."""
    N, H, W, _ = frames.shape
    D = scale
    h, w = scaled_shape(H, W, D)
    dev = frames.device
    l, r, t, b = [int(p) for p in pads]
    if N == 0:
        return torch.empty((0, 3, h + t + b, w + l + r), dtype=torch.float32, device=dev)
    x = frames.permute(0, 3, 1, 2).to(torch.int32)
    x = F.pad(x, [0, w * D - W, 0, h * D - H])  # zeros: they add nothing to a partial cell's sum
    sums = x.reshape(N, 3, h, D, w, D).sum(dim=(3, 5))
    rows = (H - torch.arange(h, device=dev) * D).clamp(max=D)
    cols = (W - torch.arange(w, device=dev) * D).clamp(max=D)
    counts = rows[:, None] * cols[None, :]
    out = sums.float() / counts.float()
    return F.pad(out, [l, r, t, b], mode="replicate")


def _axis_taps(n_out: int, D: int, n: int, dev):
    """Output indices 0..n_out-1 of one axis over n samples -> (i0, i1 int64, weight of i1 fp32)."""
    x = torch.arange(n_out, dtype=torch.int64, device=dev)
    q = x // D
    r = x % D
    t = 2 * r + 1 - D
    neg = t < 0
    i0 = torch.where(neg, q - 1, q)
    num = torch.where(neg, t + 2 * D, t)
    # a tensor divisor: a true division per element (a Python scalar may become a multiplication by 1 / (2D))
    f = num.float() / torch.full((n_out,), 2 * D, dtype=torch.float32, device=dev)
    f = torch.where((i0 < 0) | (i0 >= n - 1), torch.zeros((), dtype=torch.float32, device=dev), f)
    i0 = i0.clamp(0, n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, f


def upscale_flow_ref(flow: torch.Tensor, scale: int, left: int, top: int, w: int, h: int, H: int,
                     W: int) -> torch.Tensor:
    """fp32 (B, 2, hp, wp), the unpadded image at [top, top + h) x [left, left + w) -> fp32 (B, 2, H, W).

    Every line is one rounding step of the kernel: no ``lerp``, ``F.interpolate`` or ``grid_sample``,
    nothing that could fuse or re-associate."""
    D = scale
    dev = flow.device
    img = flow[:, :, top:top + h, left:left + w]
    y0, y1, fy = _axis_taps(H, D, h, dev)
    x0, x1, fx = _axis_taps(W, D, w, dev)
    r0, r1 = img.index_select(2, y0), img.index_select(2, y1)
    a00, a01 = r0.index_select(3, x0), r0.index_select(3, x1)
    a10, a11 = r1.index_select(3, x0), r1.index_select(3, x1)
    wx, wy = fx[None, None, None, :], fy[None, None, :, None]
    top_ = a01 - a00
    top_ = wx * top_
    top_ = a00 + top_
    bot = a11 - a10
    bot = wx * bot
    bot = a10 + bot
    s = bot - top_
    s = wy * s
    s = top_ + s
    return (s * torch.tensor(float(D), dtype=torch.float32, device=dev)).contiguous()


def ingest_frames_scaled(frames: Union[torch.Tensor, Sequence], scale: int,
                         mode: str = "sintel") -> Tuple[torch.Tensor, "InputPadder"]:
    """uint8 (N, H, W, 3) frames, or a list of (H, W, 3) arrays / tensors of one size ->
    (fp32 (N, 3, hp, wp): the frames reduced by ``scale`` to ``h x w = scaled_shape(H, W, scale)``
    and replicate padded to multiples of 8, ``InputPadder((N, 3, h, w), mode)``).

    The channel order is kept.  GPU tensors run the HIP op; everything else
    ``ingest_frames_scaled_ref``.
    """
    from ..utils.utils import InputPadder

    D = _check_scale("ingest_frames_scaled", scale)
    if not isinstance(frames, torch.Tensor):
        items = [torch.as_tensor(x) for x in frames]
        if not items or any(x.dim() != 3 or x.shape != items[0].shape for x in items):
            raise ValueError("ingest_frames_scaled: expected a non-empty list of (H, W, 3) frames of one size")
        frames = torch.stack(items)
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"ingest_frames_scaled: expected (N, H, W, 3) frames, got {tuple(frames.shape)}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"ingest_frames_scaled: expected uint8 frames, got {frames.dtype}")
    N, H, W, _ = frames.shape
    if N > 0 and (H == 0 or W == 0):
        raise ValueError(f"ingest_frames_scaled: empty frames, got {tuple(frames.shape)}")
    h, w = scaled_shape(H, W, D)
    padder = InputPadder((N, 3, h, w), mode=mode)
    if use_native(frames):
        l, r, t, b = padder._pad
        return ops().ingest_frames_scaled(frames.contiguous(), D, l, r, t, b), padder
    return ingest_frames_scaled_ref(frames, D, padder._pad), padder


def upscale_flow(flow: torch.Tensor, padder: "InputPadder", scale: int, size: Sequence[int]) -> torch.Tensor:
    """The model's flow (B, 2, hp, wp) on the padded low-resolution frame of ``padder`` (the one
    ``ingest_frames_scaled`` returned) -> fp32 (B, 2, H, W), the flow of the unpadded camera frame
    ``size = (H, W)`` in its pixel units.  GPU tensors run the HIP op; everything else
    ``upscale_flow_ref``.  The input is only read; the result is a new tensor.
    """
    D = _check_scale("upscale_flow", scale)
    if not isinstance(flow, torch.Tensor) or flow.dim() != 4 or flow.shape[1] != 2:
        shape = tuple(flow.shape) if hasattr(flow, "shape") else type(flow).__name__
        raise ValueError(f"upscale_flow: expected a (B, 2, hp, wp) tensor, got {shape}")
    if not flow.dtype.is_floating_point:
        raise ValueError(f"upscale_flow: expected a floating-point flow, got {flow.dtype}")
    if len(size) != 2:
        raise ValueError(f"upscale_flow: expected size = (H, W), got {tuple(size)}")
    H, W = int(size[0]), int(size[1])
    h, w = int(padder.ht), int(padder.wd)
    l, r, t, b = padder._pad
    if H <= 0 or W <= 0 or scaled_shape(H, W, D) != (h, w):
        raise ValueError(f"upscale_flow: a {H} x {W} frame reduced by {D} is not the padder's {h} x {w}")
    if tuple(flow.shape[-2:]) != (h + t + b, w + l + r):
        raise ValueError(f"upscale_flow: expected the padded {h + t + b} x {w + l + r} flow, got "
                         f"{tuple(flow.shape[-2:])}")
    f = flow.detach().float().contiguous()
    if use_native(f):
        return ops().upscale_flow(f, D, l, t, w, h, H, W)
    return upscale_flow_ref(f, D, l, t, w, h, H, W)
