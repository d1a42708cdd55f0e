"""The training augmentation as one HIP op: colour jitter, occlusion eraser and the resize / flip /
crop warp of ``data/augment.py`` on a padded uint8 batch.

``augment_batch`` takes the decoded batch and the parameters ``BatchAugmentor.draw`` drew, packs
the parameters into one fp32 and one int32 row per sample (the layout of ``csrc/kernel_abi.h``,
``kAug*``) and runs ``raft_amd::augment_batch`` (csrc/augment.hip): one memset and three launches
on the current stream, no host read-back.  The uint8 batch is read once inside each sample's
region, the jittered pair is kept as one dword per pixel, and only the crops are written.

With ``valid`` it runs ``raft_amd::augment_batch_sparse``, the same memset and launches: the flow
and valid of a sparse sample (KITTI, HD1K) are the scatter of its valid pixels to their rounded
positions, ``BatchAugmentor._sparse_flow``, bitwise; which samples are sparse and which are resized
travels as one int32 per sample (``pack_flags``).

``BatchAugmentor.apply`` in torch ops is the CPU path and the oracle: jitter and eraser agree
with it bitwise (on the CPU, whose division is IEEE), the bilinear warp to within one uint8 level
at a few pixels in ten thousand.  There is no torch fallback here: without the extension a GPU
call raises.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from ._ext import ops

# floats and ints per sample: kAugPF, kAugPI of csrc/kernel_abi.h
PF, PI = 10, 24


def pack_params(params: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The drawn parameters of ``BatchAugmentor.draw`` -> (pf (B, 10) fp32, pi (B, 24) int32) on
    their device: f1, f2, sx, sy and o1, o2, asym, active boxes, the two boxes, rh, rw, hflip,
    vflip, x0, y0."""
    p = params
    col = lambda t: t.view(-1, 1)  # noqa: E731
    pf = torch.cat([p["f1"].float(), p["f2"].float(), col(p["sx"].float()), col(p["sy"].float())], 1)
    nbox = torch.where(p["erase"], p["nbox"], torch.zeros_like(p["nbox"]))
    pi = torch.cat([p["o1"], p["o2"], col(p["asym"].long()), col(nbox), p["boxes"].reshape(-1, 8), col(p["rh"]),
                    col(p["rw"]), col(p["hflip"].long()), col(p["vflip"].long()), col(p["x0"]), col(p["y0"])], 1)
    assert pf.shape[1] == PF and pi.shape[1] == PI, (pf.shape, pi.shape)
    return pf.contiguous(), pi.to(torch.int32).contiguous()


# bits of a sample's flags: kAugSparse, kAugResize of csrc/kernel_abi.h
SPARSE, RESIZE = 1, 2


def pack_flags(params: Dict[str, torch.Tensor]) -> torch.Tensor:
    """``params["sparse"]`` and ``params["resize"]`` -> flags (B) int32 on their device: bit 0 the
    sample is sparse, bit 1 it is resized."""
    return (params["sparse"].to(torch.int32) * SPARSE + params["resize"].to(torch.int32) * RESIZE).contiguous()


def augment_batch(img1: torch.Tensor, img2: torch.Tensor, flow: torch.Tensor, size: torch.Tensor,
                  params: Dict[str, torch.Tensor], crop: Sequence[int], valid: Optional[torch.Tensor] = None):
    """uint8 ``img1, img2`` (B, Hm, Wm, 3), fp32 ``flow`` (B, Hm, Wm, 2), ``size`` (B, 2) and the
    drawn ``params``, all on one GPU -> fp32 ``img1, img2`` (B, 3, ch, cw), ``flow`` (B, 2, ch, cw),
    ``valid`` (B, ch, cw).  Without ``valid`` every sample is treated as dense.  With ``valid``
    (B, Hm, Wm), the samples that ``params["sparse"]`` marks take flow and valid from the scatter
    of their pixels with ``valid >= 1``."""
    if not img1.is_cuda:
        raise ValueError("augment_batch runs the HIP op and needs GPU tensors; BatchAugmentor.apply is the CPU path")
    pf, pi = pack_params(params)
    ch, cw = crop
    if valid is None:
        return ops().augment_batch(img1.contiguous(), img2.contiguous(), flow.float().contiguous(),
                                   size.long().contiguous(), pf, pi, int(ch), int(cw))
    return ops().augment_batch_sparse(img1.contiguous(), img2.contiguous(), flow.float().contiguous(),
                                      valid.float().contiguous(), size.long().contiguous(), pf, pi, pack_flags(params),
                                      int(ch), int(cw))
