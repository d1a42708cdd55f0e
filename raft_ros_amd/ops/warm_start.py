"""Warm start for video: forward-project the previous pair's low-resolution flow.

RAFT's warm start feeds the next pair ``flow_init`` = the previous ``flow_low`` splatted
forward along itself, holes filled by the nearest projected point (reference
``forward_interpolate``, core/utils/utils.py:26-54: two scipy ``griddata`` calls on the host).
On the GPU this is the HIP op ``raft_amd::forward_splat_nearest`` (csrc/forward_splat.hip):
the frame-to-frame chain stays on the device, with no host synchronisation.  It is exact
(fp64 distances) and deterministic (ties go to the lowest source index), where scipy leaves
ties unspecified; ``reference.forward_splat_nearest_ref`` is its brute-force oracle.
"""
from __future__ import annotations

import torch

from ._ext import ops, use_native


def forward_splat_nearest(flow: torch.Tensor) -> torch.Tensor:
    """(2, H, W) or (B, 2, H, W) flow -> the same shape, fp32, on ``flow``'s device.

    GPU tensors run the HIP op; everything else goes through ``forward_interpolate`` (scipy)
    image by image.
    """
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise ValueError(f"forward_splat_nearest: expected (2, H, W) or (B, 2, H, W), got {tuple(flow.shape)}")
    squeeze = flow.dim() == 3
    f = flow[None] if squeeze else flow
    if use_native(f):
        out = ops().forward_splat_nearest(f.detach().float().contiguous())
    else:
        from ..utils.utils import forward_interpolate

        out = torch.stack([forward_interpolate(x) for x in f]).to(flow.device)
    return out[0] if squeeze else out
