"""Corner seeds: the Shi-Tomasi corner of every grid cell, where the point tracker starts its points.

``ops/track.py`` puts a fresh point at the centre of its cell, which often lies on sky, road or a
wall: there the flow is least constrained and a triangulator gains nothing.  ``corner_seeds`` finds,
per cell of the tracker's grid, the pixel with the largest smaller eigenvalue of the structure
tensor (what ``goodFeaturesToTrack`` ranks by), in integer arithmetic so that every path agrees
bitwise.

* ``corner_seeds``: GPU tensors run the HIP op ``raft_amd::corner_seeds`` (csrc/corner_seeds.hip):
  three launches on the current stream, nothing read back.  Everything else runs the reference.
* ``corner_seeds_ref``: the same sequence in integer torch ops; the CPU path and the tests' oracle.
* ``slot_scores``: the score every slot of the tracker was born with, carried across steps.

Per image of ``frames`` (B, H, W, 3) uint8, the roi being the pixels ``[0, w) x [0, h)``::

    g     = (c0 + 2 c1 + c2 + 2) >> 2                  symmetric in the outer channels: RGB = BGR
    Ix    = (g[y-1,x+1] + 2 g[y,x+1] + g[y+1,x+1]) - (the same at x-1)     coordinates clamped into
    Iy    = (g[y+1,x-1] + 2 g[y+1,x] + g[y+1,x+1]) - (the same at y-1)     the image
    a,b,c = the sums of Ix^2, Ix Iy, Iy^2 over the 3 x 3 window, at clamped coordinates
    score = (a + c) - isqrt((a - c)^2 + 4 b^2)         twice the smaller eigenvalue, rounded up
    a candidate of cell (y // S, x // S) is a roi pixel with margin <= x % S, y % S <= S - 1 - margin
    winner of a cell: the largest score, among equals the lowest y * w + x
    seed = origin + the winner when its score > min_score, else origin + the cell's clamped centre
    score = the winner's, -1 for a cell without candidates
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from ._ext import ops, use_native
from .track import _seed_xy, grid_shape

SCORE_MAX = 2 * 9 * 1020 * 1020  # a + c at its largest: 18 727 200 < 2^25


def _check(frames, S, roi_size, origin, margin, min_score) -> Tuple[int, int, int, int, int, int, int]:
    """-> (S, w, h, left, top, margin, min_score) as ints, or ValueError."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        got = frames.dtype if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"corner_seeds: expected frames as a uint8 tensor, got {got}")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"corner_seeds: expected frames of shape (B, H, W, 3), got {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError("corner_seeds: frames must be contiguous")
    _, H, W, _ = frames.shape
    if H < 1 or W < 1:
        raise ValueError(f"corner_seeds: empty frames {tuple(frames.shape)}")
    if isinstance(S, bool) or int(S) != S or int(S) < 1:
        raise ValueError(f"corner_seeds: the cell size must be an integer of at least 1, got {S!r}")
    S = int(S)
    if S >= 2 ** 31:
        raise ValueError(f"corner_seeds: the cell size {S} is too large")
    w, h = (W, H) if roi_size is None else (int(v) for v in roi_size)
    if not (1 <= w <= W and 1 <= h <= H):
        raise ValueError(f"corner_seeds: the roi size (w, h) = {(w, h)} must lie inside the {H} x {W} frame")
    if H * W >= 2 ** 31:
        raise ValueError(f"corner_seeds: frame of {H} x {W} pixels too large")
    left, top = (int(v) for v in origin)
    if not (-2 ** 23 <= left and left + w <= 2 ** 23 and -2 ** 23 <= top and top + h <= 2 ** 23):
        raise ValueError(f"corner_seeds: the origin {(left, top)} leaves the range fp32 holds exactly")
    margin = S // 4 if margin is None else int(margin)
    if margin < 0 or 2 * margin > S - 1:
        raise ValueError(f"corner_seeds: the margin needs 0 <= 2 * margin <= S - 1, got margin {margin} with S {S}")
    if isinstance(min_score, float) and int(min_score) != min_score:
        raise ValueError(f"corner_seeds: min_score is an integer in the score's units, got {min_score!r}")
    min_score = int(min_score)
    if not -2 ** 62 <= min_score < 2 ** 62:
        raise ValueError(f"corner_seeds: min_score {min_score} out of range")
    Gy, Gx = grid_shape((0, 0, w, h), S)
    if frames.shape[0] * Gy * Gx >= 2 ** 31:
        raise ValueError(f"corner_seeds: B * N = {frames.shape[0] * Gy * Gx} too large")
    return S, w, h, left, top, margin, min_score


def corner_score_ref(frames: torch.Tensor) -> torch.Tensor:
    """The score of every pixel: (B, H, W) int64.  Every intermediate is an exact integer."""
    B, H, W, _ = frames.shape
    f = frames.long()
    g = (f[..., 0] + 2 * f[..., 1] + f[..., 2] + 2) >> 2
    dev = frames.device
    ys, xs = torch.arange(H, device=dev), torch.arange(W, device=dev)

    def shifted(t, dy, dx):  # t[y + dy, x + dx] at clamped coordinates
        return t[:, (ys + dy).clamp(0, H - 1)][:, :, (xs + dx).clamp(0, W - 1)]

    ix = (shifted(g, -1, 1) + 2 * shifted(g, 0, 1) + shifted(g, 1, 1)) - \
         (shifted(g, -1, -1) + 2 * shifted(g, 0, -1) + shifted(g, 1, -1))
    iy = (shifted(g, 1, -1) + 2 * shifted(g, 1, 0) + shifted(g, 1, 1)) - \
         (shifted(g, -1, -1) + 2 * shifted(g, -1, 0) + shifted(g, -1, 1))
    xx, xy, yy = ix * ix, ix * iy, iy * iy
    a, b, c = torch.zeros_like(xx), torch.zeros_like(xx), torch.zeros_like(xx)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            a, b, c = a + shifted(xx, dy, dx), b + shifted(xy, dy, dx), c + shifted(yy, dy, dx)
    d = (a - c) * (a - c) + 4 * b * b  # < 2^53: exact as a double
    r = d.double().sqrt().floor().long()
    r = torch.where(r * r > d, r - 1, r)  # whatever the library's root rounds to,
    r = torch.where((r + 1) * (r + 1) <= d, r + 1, r)  # r is the integer floor
    return (a + c) - r


def corner_seeds_ref(frames: torch.Tensor, S: int, roi_size: Optional[Sequence[int]] = None,
                     origin: Sequence[int] = (0, 0), margin: Optional[int] = None, min_score: int = 0):
    """``corner_seeds`` as integer torch ops -> (seeds (B, N, 2) fp32, score (B, N) int32).

    The per-cell winner is an ``amax`` scatter of ``score << 32 | (0xffffffff - (y * w + x))``, the
    kernel's key; 0 marks a pixel that is no candidate and a cell without one."""
    S, w, h, left, top, margin, min_score = _check(frames, S, roi_size, origin, margin, min_score)
    B = frames.shape[0]
    dev = frames.device
    roi = (left, top, w, h)
    Gy, Gx = grid_shape(roi, S)
    N = Gy * Gx
    if B == 0:
        return (torch.empty((0, N, 2), dtype=torch.float32, device=dev),
                torch.empty((0, N), dtype=torch.int32, device=dev))
    score = corner_score_ref(frames)[:, :h, :w]
    ys, xs = torch.arange(h, device=dev), torch.arange(w, device=dev)
    oy, ox = ys % S, xs % S
    cand = ((oy >= margin) & (oy <= S - 1 - margin))[:, None] & ((ox >= margin) & (ox <= S - 1 - margin))[None, :]
    idx = ys[:, None] * w + xs[None, :]
    cell = (ys // S)[:, None] * Gx + (xs // S)[None, :]
    key = torch.where(cand[None], (score << 32) | (0xffffffff - idx)[None], torch.zeros_like(score))
    keys = torch.zeros((B, N), dtype=torch.int64, device=dev)
    keys = keys.scatter_reduce(1, cell.reshape(1, h * w).expand(B, h * w), key.reshape(B, h * w), reduce="amax",
                               include_self=True)
    has = keys != 0
    best = keys >> 32
    widx = 0xffffffff - (keys & 0xffffffff)
    take = has & (best > min_score)
    centre = _seed_xy(roi, S, dev)  # fp32 of exact integers, the origin included
    corner = torch.stack([left + widx % w, top + widx // w], dim=-1).float()
    seeds = torch.where(take[..., None], corner, centre[None].expand(B, N, 2))
    out_score = torch.where(has, best, torch.full_like(best, -1)).to(torch.int32)
    return seeds.contiguous(), out_score


def corner_seeds(frames: torch.Tensor, S: int, roi_size: Optional[Sequence[int]] = None,
                 origin: Sequence[int] = (0, 0), margin: Optional[int] = None, min_score: int = 0):
    """The corner seed of every cell -> (seeds (B, N, 2) fp32 (x, y), score (B, N) int32).

    ``frames`` (B, H, W, 3) uint8, contiguous (the layout ``ingest_frames`` takes; the channel order
    does not matter).  The roi is the pixels ``[0, w) x [0, h)`` of the frame, ``roi_size = (w, h)``
    (default: the whole frame), tiled by the ``N = Gy * Gx`` cells of size ``S`` of
    ``track.grid_shape``; ``origin = (left, top)`` is added to every seed, so that
    ``roi = (left, top, w, h)`` is the tracker's.  ``margin`` (default ``S // 4``) keeps the seeds
    away from the borders of their cells; ``min_score`` (an integer in the score's units, default
    0) sends the cells without a corner back to their centre.  ``score`` is the best candidate's
    score, -1 for a (partial) cell without candidates."""
    S, w, h, left, top, margin, min_score = _check(frames, S, roi_size, origin, margin, min_score)
    if use_native(frames):
        return tuple(ops().corner_seeds(frames, S, w, h, left, top, margin, min_score))
    return corner_seeds_ref(frames, S, (w, h), (left, top), margin, min_score)


def slot_scores(pos: torch.Tensor, age: torch.Tensor, kept: Optional[torch.Tensor], cell_score: torch.Tensor,
                roi: Sequence[int], S: int) -> torch.Tensor:
    """The score every slot's point was born with: (B, N) int32.

    A slot with ``age == 0`` holds a point that has just been seeded: it sits on the seed of a
    cell, inside that cell, and takes that cell's entry of ``cell_score`` (B, N); any other slot
    keeps its entry of ``kept`` (None: a fresh grid, every slot is new)."""
    left, top, w, h = (int(v) for v in roi)
    _, Gx = grid_shape(roi, int(S))
    cell = ((pos[..., 1].long() - top) // int(S)) * Gx + (pos[..., 0].long() - left) // int(S)
    born = cell_score.gather(1, cell.clamp(0, cell_score.shape[1] - 1))
    return born if kept is None else torch.where(age == 0, born, kept)
