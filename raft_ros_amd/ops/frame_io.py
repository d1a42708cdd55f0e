"""Device-side frame path: what the ROS node and demo.py do around the model.

* ``flow_to_image``: the Middlebury colour coding of ``utils/flow_viz.flow_to_image`` (reference
  core/utils/flow_viz.py) of a flow that lives on the GPU, through the HIP op
  ``raft_amd::flow_to_image`` (csrc/flow_color.hip): only the uint8 image has to cross to the
  host.  The numpy path and the op agree to one level on rare pixels (the last bit of
  ``arctan2``).
* ``ingest_frames``: camera frames as the camera delivers them (uint8, HWC) to the model's
  padded fp32 CHW input through ``raft_amd::ingest_frames``, bitwise what
  ``InputPadder.pad(frames.permute(0, 3, 1, 2).float())`` gives: the upload is a quarter of the
  fp32 one and the conversion and the replicate padding are one launch.

Both run on the current stream without host synchronisation.  CPU tensors go through the
numpy / torch code the ops replace.
"""
from __future__ import annotations

from typing import TYPE_CHECKING, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._ext import ops, use_native

if TYPE_CHECKING:  # utils.utils imports ops.reference: import it where it is used
    from ..utils.utils import InputPadder


def flow_to_image(flow: torch.Tensor, clip_flow: Optional[float] = None, convert_to_bgr: bool = False) -> torch.Tensor:
    """(2, H, W) or (B, 2, H, W) flow -> (H, W, 3) or (B, H, W, 3) uint8 on ``flow``'s device.

    Each image is normalised by its own largest radius.  GPU tensors run the HIP op; everything
    else goes through ``utils.flow_viz.flow_to_image`` image by image.
    """
    if not isinstance(flow, torch.Tensor) or flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        shape = tuple(flow.shape) if hasattr(flow, "shape") else type(flow).__name__
        raise ValueError(f"flow_to_image: expected a (2, H, W) or (B, 2, H, W) tensor, got {shape}")
    if not flow.dtype.is_floating_point:
        raise ValueError(f"flow_to_image: expected a floating-point flow, got {flow.dtype}")
    squeeze = flow.dim() == 3
    f = flow[None] if squeeze else flow
    if use_native(f):
        clip = None if clip_flow is None else float(clip_flow)
        out = ops().flow_to_image(f.detach().float().contiguous(), clip, bool(convert_to_bgr))
    else:
        from ..utils import flow_viz

        imgs = [flow_viz.flow_to_image(x.detach().float().permute(1, 2, 0).cpu().numpy(), clip_flow, convert_to_bgr)
                for x in f]
        out = torch.from_numpy(np.stack(imgs)) if imgs else torch.empty((0,) + tuple(f.shape[2:]) + (3,),
                                                                        dtype=torch.uint8)
        out = out.to(flow.device)
    return out[0] if squeeze else out


def ingest_frames(frames: Union[torch.Tensor, Sequence], mode: str = "sintel") -> Tuple[torch.Tensor, "InputPadder"]:
    """uint8 (N, H, W, 3) frames, or a list of (H, W, 3) arrays / tensors of one size ->
    (fp32 (N, 3, Hp, Wp) replicate padded to multiples of 8, the ``InputPadder`` that undoes it).

    The channel order is kept.  GPU tensors run the HIP op; everything else ``InputPadder.pad``.
    """
    from ..utils.utils import InputPadder

    if not isinstance(frames, torch.Tensor):
        items = [torch.as_tensor(x) for x in frames]
        if not items or any(x.dim() != 3 or x.shape != items[0].shape for x in items):
            raise ValueError("ingest_frames: expected a non-empty list of (H, W, 3) frames of one size")
        frames = torch.stack(items)
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"ingest_frames: expected (N, H, W, 3) frames, got {tuple(frames.shape)}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"ingest_frames: expected uint8 frames, got {frames.dtype}")
    N, H, W, _ = frames.shape
    padder = InputPadder((N, 3, H, W), mode=mode)
    if use_native(frames):
        l, r, t, b = padder._pad
        return ops().ingest_frames(frames.contiguous(), l, r, t, b), padder
    return padder.pad(frames.permute(0, 3, 1, 2).float())[0], padder
