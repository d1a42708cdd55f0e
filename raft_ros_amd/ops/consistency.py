"""Forward-backward consistency of a flow pair: where can the forward flow be trusted?

RAFT has no confidence output.  The standard answer computes the flow in both directions, follows
the forward flow and reads the backward flow there: the two should cancel.  Where they do not, the
pixel is occluded or mismatched (class 1); where the forward flow leaves the frame nothing can be
said (class 2); everything else is consistent (class 0).

* ``fb_consistency``: GPU tensors run the HIP op ``raft_amd::fb_consistency``
  (csrc/fb_consistency.hip), one memset and one launch on the current stream without host
  synchronisation; everything else runs ``fb_consistency_ref``.
* ``fb_consistency_ref``: the same arithmetic as plain torch tensor ops, one op per step and in the
  kernel's order, so that the two agree bitwise.  It is the CPU path and the tests' oracle.

Per pixel (x, y), all in fp32::

    u, v = fw[:, y, x];  px = x + u;  py = y + v
    outside [0, W-1] x [0, H-1] (NaN is outside):  occ = 2, err2 = +inf
    x0 = floor(px); y0 = floor(py); fx = px - x0; fy = py - y0
    x1 = min(x0 + 1, W-1); y1 = min(y0 + 1, H-1)
    per component c of bw:  top = a00 + fx * (a01 - a00);  bot = a10 + fx * (a11 - a10)
                            s_c = top + fy * (bot - top)
    err2 = (u + s_0)^2 + (v + s_1)^2
    occ  = 0 if err2 <= alpha1 * ((u^2 + v^2) + (s_0^2 + s_1^2)) + alpha2 else 1      (NaN -> 1)
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from ._ext import ops, use_native

ALPHA1 = 0.01  # the usual values of this criterion
ALPHA2 = 0.5
# the mask as a mono image (the node's /raft_occlusion, demo.py's occ_%04d.png): OCC_LEVELS[occ]
OCC_LEVELS = np.array([0, 128, 255], dtype=np.uint8)


def fb_consistency_ref(flow_fw: torch.Tensor, flow_bw: torch.Tensor, alpha1: float = ALPHA1,
                       alpha2: float = ALPHA2) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp32 (B, 2, H, W) flows -> occ (B, H, W) uint8, err2 (B, H, W) fp32, counts (B, 2) int32.

    Every line is one rounding step of the kernel: no ``lerp``, ``addcmul`` or ``grid_sample``,
    nothing that could fuse or re-associate."""
    B, _, H, W = flow_fw.shape
    dev = flow_fw.device
    if B == 0 or H * W == 0:
        return (torch.empty((B, H, W), dtype=torch.uint8, device=dev),
                torch.empty((B, H, W), dtype=torch.float32, device=dev),
                torch.zeros((B, 2), dtype=torch.int32, device=dev))
    u, v = flow_fw[:, 0], flow_fw[:, 1]
    px = torch.arange(W, dtype=torch.float32, device=dev)[None, None, :] + u
    py = torch.arange(H, dtype=torch.float32, device=dev)[None, :, None] + v
    inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)  # a NaN compares false
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    pxs, pys = torch.where(inside, px, zero), torch.where(inside, py, zero)  # outside: sample pixel 0, dropped below
    x0f, y0f = pxs.floor(), pys.floor()
    fx, fy = pxs - x0f, pys - y0f
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    planes = flow_bw.reshape(B, 2, H * W)

    def at(yy, xx):  # both components of bw at integer positions: (B, 2, H, W)
        idx = (yy * W + xx).reshape(B, 1, H * W).expand(B, 2, H * W)
        return torch.gather(planes, 2, idx).reshape(B, 2, H, W)

    a00, a01, a10, a11 = at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1)
    wx, wy = fx[:, None], fy[:, None]
    top = a01 - a00
    top = wx * top
    top = a00 + top
    bot = a11 - a10
    bot = wx * bot
    bot = a10 + bot
    s = bot - top
    s = wy * s
    s = top + s
    s0, s1 = s[:, 0], s[:, 1]
    du, dv = u + s0, v + s1
    err2 = du * du + dv * dv
    a1 = torch.tensor(alpha1, dtype=torch.float32, device=dev)
    a2 = torch.tensor(alpha2, dtype=torch.float32, device=dev)
    thr = (u * u + v * v) + (s0 * s0 + s1 * s1)
    thr = a1 * thr
    thr = thr + a2
    occ = (~(err2 <= thr)).to(torch.uint8)  # a NaN error is inconsistent
    occ = torch.where(inside, occ, torch.full((), 2, dtype=torch.uint8, device=dev))
    err2 = torch.where(inside, err2, torch.full((), float("inf"), dtype=torch.float32, device=dev))
    counts = torch.stack([(occ == 1).sum(dim=(1, 2)), (occ == 2).sum(dim=(1, 2))], dim=1).to(torch.int32)
    return occ, err2, counts


def fb_consistency(flow_fw: torch.Tensor, flow_bw: torch.Tensor, alpha1: float = ALPHA1,
                   alpha2: float = ALPHA2) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(2, H, W) or (B, 2, H, W) forward and backward flow -> (occ, err2, counts) on their device.

    ``occ`` uint8 (B, H, W): 0 consistent, 1 inconsistent, 2 the forward flow leaves the frame;
    ``err2`` fp32 (B, H, W): the squared forward-backward error, +inf for class 2; ``counts`` int32
    (B, 2): the pixels of class 1 and of class 2 per image.  The unbatched form drops B.
    """
    for name, f in (("flow_fw", flow_fw), ("flow_bw", flow_bw)):
        if not isinstance(f, torch.Tensor) or f.dim() not in (3, 4) or f.shape[-3] != 2:
            shape = tuple(f.shape) if hasattr(f, "shape") else type(f).__name__
            raise ValueError(f"fb_consistency: expected {name} as a (2, H, W) or (B, 2, H, W) tensor, got {shape}")
        if not f.dtype.is_floating_point:
            raise ValueError(f"fb_consistency: expected a floating-point {name}, got {f.dtype}")
    if flow_fw.shape != flow_bw.shape:
        raise ValueError(f"fb_consistency: flow_fw and flow_bw differ in shape: {tuple(flow_fw.shape)} and "
                         f"{tuple(flow_bw.shape)}")
    if flow_fw.device != flow_bw.device:
        raise ValueError(f"fb_consistency: flow_fw is on {flow_fw.device}, flow_bw on {flow_bw.device}")
    squeeze = flow_fw.dim() == 3
    fw = (flow_fw[None] if squeeze else flow_fw).detach().float().contiguous()
    bw = (flow_bw[None] if squeeze else flow_bw).detach().float().contiguous()
    if use_native(fw):
        occ, err2, counts = ops().fb_consistency(fw, bw, float(alpha1), float(alpha2))
    else:
        occ, err2, counts = fb_consistency_ref(fw, bw, float(alpha1), float(alpha2))
    return (occ[0], err2[0], counts[0]) if squeeze else (occ, err2, counts)
