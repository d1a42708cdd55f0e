"""Point tracks: a grid of points with stable ids followed through the flow, on the device.

A picture of the flow is what a viewer wants; a VIO / SLAM front end wants correspondences: points
with ids, where each was in the previous frame, and how long it has lived (what a KLT tracker
delivers).  The region of interest ``roi = (left, top, w, h)`` of the flow frame is tiled by cells
of size ``S``; every cell holds exactly one point.  One step advances every point by the forward
flow, drops the ones that leave the roi (status 2) or fail the forward-backward check of
``ops/consistency.py`` (status 1), keeps the oldest point of a crowded cell (the others: status 3)
and puts a fresh point with a new id at the seed position of every cell left empty.

* ``track_points``: GPU tensors run the HIP op ``raft_amd::track_points``
  (csrc/track_points.hip): three launches on the current stream, nothing read back.
  Everything else runs ``track_points_ref``.
* ``track_points_ref``: the same sequence as plain torch ops, one op per rounding step and in the
  kernel's order, so that the two agree bitwise.  It is the CPU path and the tests' oracle.
* ``seed_points``: the initial state, slot ``j`` at the seed of cell ``j``.
* ``PointTracker``: the state kept on the device across pairs.

Per slot, all in fp32 (``fw`` and ``bw`` are read bilinearly with ``fb_consistency``'s formula)::

    p = pos;  outside [left, left+w-1] x [top, top+h-1] (NaN is outside):  status 2, err2 = +inf
    f = fw(p);  q = p + f;  q outside the roi:                              status 2, err2 = +inf
    with bw:  s = bw(q);  err2 = (f0 + s0)^2 + (f1 + s1)^2
              status 1 unless err2 <= alpha1 * ((f0^2 + f1^2) + (s0^2 + s1^2)) + alpha2  (NaN -> 1)
    without:  err2 = 0
    a survivor claims cell ((floor(qy) - top) // S) * Gx + (floor(qx) - left) // S with the key
    (0xffffffff - age) << 32 | slot; the smallest key owns the cell (the oldest, then the lowest slot)
    owner: status 0, pos_out = q, prev = p, id kept, age + 1;  other survivors: status 3
    the k-th slot (in slot order) whose status is not 0 takes the k-th unowned cell (in cell order):
    pos_out = its seed (the cell's clamped centre, or seeds[b, cell]), prev = (NaN, NaN),
    id = epoch * N + slot, age = 0
    epoch_out = epoch + 1
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from ._ext import ops, use_native
from .consistency import ALPHA1, ALPHA2

Roi = Tuple[int, int, int, int]


def grid_shape(roi: Sequence[int], S: int) -> Tuple[int, int]:
    """(Gy, Gx): the cells that tile the roi; the ones on the right and lower edge may be partial."""
    _, _, w, h = roi
    return -(-h // S), -(-w // S)


def _check_grid(roi, S) -> Roi:
    roi = tuple(int(v) for v in roi)
    if len(roi) != 4:
        raise ValueError(f"track_points: the roi is (left, top, w, h), got {roi}")
    if int(S) < 1:
        raise ValueError(f"track_points: the cell size must be at least 1, got {S}")
    if roi[2] < 1 or roi[3] < 1 or roi[0] < 0 or roi[1] < 0:
        raise ValueError(f"track_points: the roi (left, top, w, h) needs left, top >= 0 and w, h >= 1, got {roi}")
    return roi


def _seed_xy(roi: Roi, S: int, device) -> torch.Tensor:
    """The fp32 seed position (x, y) of every cell: (N, 2)."""
    left, top, w, h = roi
    Gy, Gx = grid_shape(roi, S)
    sx = left + (torch.arange(Gx, dtype=torch.int64, device=device) * S + S // 2).clamp(max=w - 1)
    sy = top + (torch.arange(Gy, dtype=torch.int64, device=device) * S + S // 2).clamp(max=h - 1)
    return torch.stack([sx[None, :].expand(Gy, Gx), sy[:, None].expand(Gy, Gx)], dim=-1).reshape(Gy * Gx, 2).float()


def _check_seeds(seeds, B: int, N: int, device) -> None:
    if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.float32:
        raise ValueError(f"track_points: expected seeds as a torch.float32 tensor, got "
                         f"{seeds.dtype if isinstance(seeds, torch.Tensor) else type(seeds).__name__}")
    if tuple(seeds.shape) != (B, N, 2):
        raise ValueError(f"track_points: expected seeds of shape {(B, N, 2)}, got {tuple(seeds.shape)}")
    if device is not None and seeds.device != torch.device(device):
        raise ValueError(f"track_points: seeds are on {seeds.device}, the state on {device}")
    if not seeds.is_contiguous():
        raise ValueError("track_points: seeds must be contiguous")


def seed_points(B: int, roi: Sequence[int], S: int, device=None, seeds: Optional[torch.Tensor] = None):
    """The initial state (pos (B, N, 2) fp32, ids (B, N) int64, age (B, N) int32, epoch (1,) int64):
    slot ``j`` at the seed of cell ``j`` (``seeds[:, j]`` when ``seeds`` (B, N, 2) fp32 is given, else
    the cell's clamped centre), ``ids = j``, ``age = 0``, ``epoch = 1``."""
    roi = _check_grid(roi, S)
    S = int(S)
    if seeds is None:
        centres = _seed_xy(roi, S, device)
        N = centres.shape[0]
        pos = centres[None].expand(B, N, 2).contiguous()
    else:
        Gy, Gx = grid_shape(roi, S)
        N = Gy * Gx
        device = seeds.device if device is None and isinstance(seeds, torch.Tensor) else device
        _check_seeds(seeds, B, N, device)
        pos = seeds.clone()
    ids = torch.arange(N, dtype=torch.int64, device=device)[None].expand(B, N).contiguous()
    age = torch.zeros((B, N), dtype=torch.int32, device=device)
    epoch = torch.ones((1,), dtype=torch.int64, device=device)
    return pos, ids, age, epoch


def _bilinear(planes: torch.Tensor, x: torch.Tensor, y: torch.Tensor, H: int, W: int):
    """Both components of the flow ``planes`` (B, 2, H * W) at the points (x, y) (B, N) inside the
    frame: two (B, N) tensors.  Every line is one rounding step of the kernel."""
    B, N = x.shape
    x0f, y0f = x.floor(), y.floor()
    fx, fy = x - x0f, y - y0f
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)

    def at(yy, xx):
        return torch.gather(planes, 2, (yy * W + xx)[:, None, :].expand(B, 2, N))

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
    return s[:, 0], s[:, 1]


def track_points_ref(pos: torch.Tensor, ids: torch.Tensor, age: torch.Tensor, epoch: torch.Tensor,
                     flow_fw: torch.Tensor, flow_bw: Optional[torch.Tensor] = None,
                     roi: Optional[Sequence[int]] = None, S: int = 32, alpha1: float = ALPHA1,
                     alpha2: float = ALPHA2, seeds: Optional[torch.Tensor] = None):
    """One step as torch ops -> (pos_out, prev, ids_out, age_out, epoch_out, status, err2, counts).

    Every line is one rounding step of the kernel: no ``lerp``, ``addcmul`` or ``grid_sample``,
    nothing that could fuse or re-associate.  The claim is an ``amin`` scatter on int64 keys (every
    key has its top bit set, as ``age < 2^31``, so that the signed order is the unsigned one and the
    empty key -1 is the largest), the matching of lost slots to unowned cells two ``cumsum``."""
    B, _, H, W = flow_fw.shape
    dev = flow_fw.device
    left, top_, w, h = roi = (0, 0, W, H) if roi is None else tuple(int(v) for v in roi)
    S = int(S)
    Gy, Gx = grid_shape(roi, S)
    N = Gy * Gx
    epoch_out = epoch.reshape(1) + 1
    if B == 0:
        return (pos.new_empty((0, N, 2)), pos.new_empty((0, N, 2)), ids.new_empty((0, N)), age.new_empty((0, N)),
                epoch_out, torch.empty((0, N), dtype=torch.uint8, device=dev), pos.new_empty((0, N)),
                torch.empty((0, 4), dtype=torch.int32, device=dev))
    f32 = dict(dtype=torch.float32, device=dev)
    inf = torch.full((), float("inf"), **f32)
    xlo, xhi = torch.tensor(float(left), **f32), torch.tensor(float(left + w - 1), **f32)
    ylo, yhi = torch.tensor(float(top_), **f32), torch.tensor(float(top_ + h - 1), **f32)

    def in_roi(x, y):  # a NaN compares false
        return (x >= xlo) & (x <= xhi) & (y >= ylo) & (y <= yhi)

    px, py = pos[..., 0], pos[..., 1]
    p_in = in_roi(px, py)
    # outside: sample the roi's corner, dropped below
    pxs, pys = torch.where(p_in, px, xlo), torch.where(p_in, py, ylo)
    f0, f1 = _bilinear(flow_fw.reshape(B, 2, H * W), pxs, pys, H, W)
    qx, qy = pxs + f0, pys + f1
    alive = p_in & in_roi(qx, qy)
    qxs, qys = torch.where(alive, qx, xlo), torch.where(alive, qy, ylo)
    if flow_bw is not None:
        s0, s1 = _bilinear(flow_bw.reshape(B, 2, H * W), qxs, qys, H, W)
        du, dv = f0 + s0, f1 + s1
        err2 = du * du + dv * dv
        thr = (f0 * f0 + f1 * f1) + (s0 * s0 + s1 * s1)
        thr = torch.tensor(alpha1, **f32) * thr
        thr = thr + torch.tensor(alpha2, **f32)
        ok = err2 <= thr  # a NaN error is inconsistent
    else:
        err2 = torch.zeros((B, N), **f32)
        ok = torch.ones((B, N), dtype=torch.bool, device=dev)
    err2 = torch.where(alive, err2, inf)
    status = torch.where(alive, (~ok).to(torch.uint8), torch.full((), 2, dtype=torch.uint8, device=dev))
    surv = alive & ok
    # the claim: the smallest key of a cell owns it
    slots = torch.arange(N, dtype=torch.int64, device=dev)[None].expand(B, N)
    cell = ((qys.floor().long() - top_) // S) * Gx + (qxs.floor().long() - left) // S
    key = ((-1 - age.long()) << 32) | slots
    none = torch.full((), -1, dtype=torch.int64, device=dev)
    keys = torch.full((B, N), -1, dtype=torch.int64, device=dev)
    keys = keys.scatter_reduce(1, cell, torch.where(surv, key, none), reduce="amin", include_self=True)
    owner = surv & ((keys.gather(1, cell) & 0xffffffff) == slots)
    status = torch.where(surv & ~owner, torch.full((), 3, dtype=torch.uint8, device=dev), status)
    # the k-th lost slot takes the k-th unowned cell
    lost = ~owner
    unowned = keys == none
    rank = lost.long().cumsum(1) - 1
    urank = unowned.long().cumsum(1) - 1
    free_cells = torch.zeros((B, N + 1), dtype=torch.int64, device=dev)  # column N takes the owned cells
    free_cells = free_cells.scatter(1, torch.where(unowned, urank, torch.full_like(urank, N)), slots)
    new_cell = free_cells.gather(1, torch.where(lost, rank, torch.zeros_like(rank)))
    if seeds is None:
        seeds = _seed_xy(roi, S, dev)[new_cell]  # (B, N, 2)
    else:  # the caller's seed of every cell
        seeds = seeds.gather(1, new_cell[..., None].expand(B, N, 2))
    nan = torch.full((), float("nan"), **f32)
    own2 = owner[..., None]
    pos_out = torch.where(own2, torch.stack([qx, qy], dim=-1), seeds)
    prev = torch.where(own2, pos, nan)
    ids_out = torch.where(owner, ids, epoch.reshape(1, 1) * N + slots)
    age_out = torch.where(owner, age + 1, torch.zeros_like(age))
    counts = torch.stack([(status == k).sum(dim=1) for k in range(4)], dim=1).to(torch.int32)
    return pos_out, prev, ids_out, age_out, epoch_out, status, err2, counts


def _check_args(pos, ids, age, epoch, flow_fw, flow_bw, roi, S) -> Roi:
    if not isinstance(flow_fw, torch.Tensor) or flow_fw.dim() != 4 or flow_fw.shape[1] != 2:
        shape = tuple(flow_fw.shape) if hasattr(flow_fw, "shape") else type(flow_fw).__name__
        raise ValueError(f"track_points: expected flow_fw as a (B, 2, H, W) tensor, got {shape}")
    B, _, H, W = flow_fw.shape
    roi = _check_grid((0, 0, W, H) if roi is None else roi, S)
    left, top, w, h = roi
    if left + w > W or top + h > H:
        raise ValueError(f"track_points: the roi {roi} does not lie inside the {H} x {W} frame")
    Gy, Gx = grid_shape(roi, int(S))
    N = Gy * Gx
    tensors = [("pos", pos, torch.float32, (B, N, 2)), ("ids", ids, torch.int64, (B, N)),
               ("age", age, torch.int32, (B, N)), ("flow_fw", flow_fw, torch.float32, (B, 2, H, W))]
    if flow_bw is not None:
        tensors.append(("flow_bw", flow_bw, torch.float32, (B, 2, H, W)))
    for name, t, dtype, shape in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"track_points: expected {name} as a {dtype} tensor, got "
                             f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if tuple(t.shape) != shape:
            raise ValueError(f"track_points: expected {name} of shape {shape} (a grid of {Gy} x {Gx} cells), got "
                             f"{tuple(t.shape)}")
        if t.device != flow_fw.device:
            raise ValueError(f"track_points: {name} is on {t.device}, flow_fw on {flow_fw.device}")
        if not t.is_contiguous():
            raise ValueError(f"track_points: {name} must be contiguous")
    if not isinstance(epoch, torch.Tensor) or epoch.dtype != torch.int64 or epoch.numel() != 1:
        raise ValueError("track_points: expected epoch as an int64 tensor of one element")
    if epoch.device != flow_fw.device:
        raise ValueError(f"track_points: epoch is on {epoch.device}, flow_fw on {flow_fw.device}")
    if B * N >= 2 ** 31:
        raise ValueError(f"track_points: B * N = {B * N} too large")
    if not ids.is_cuda and ids.numel() and int(ids.min()) < 0:  # the caller's contract; checked where it is free
        raise ValueError("track_points: ids must not be negative")
    return roi


def track_points(pos: torch.Tensor, ids: torch.Tensor, age: torch.Tensor, epoch: torch.Tensor,
                 flow_fw: torch.Tensor, flow_bw: Optional[torch.Tensor] = None,
                 roi: Optional[Sequence[int]] = None, S: int = 32, alpha1: float = ALPHA1, alpha2: float = ALPHA2,
                 seeds: Optional[torch.Tensor] = None):
    """One step of the point grid -> (pos_out, prev, ids_out, age_out, epoch_out, status, err2, counts).

    ``pos`` (B, N, 2) fp32 (x, y) in frame coordinates, ``ids`` (B, N) int64 >= 0, ``age`` (B, N)
    int32, ``epoch`` (1,) int64, ``flow_fw`` and optionally ``flow_bw`` (B, 2, H, W) fp32, all
    contiguous and on one device; ``roi = (left, top, w, h)`` inside the frame (default: the whole
    frame), ``N`` the cell count of the grid.  ``status`` (B, N) uint8 is the fate of the point the
    slot held on entry: 0 tracked, 1 inconsistent, 2 left the roi, 3 crowded out; ``err2`` (B, N)
    its squared forward-backward error (+inf for status 2, 0 without ``flow_bw``); ``counts``
    (B, 4) int32 the slots per status.  Slots of status 0 keep their id; all others hold a new
    point (``age = 0``, ``prev = NaN``), which starts at the clamped centre of its cell or, with
    ``seeds`` (B, N, 2) fp32 (``ops/corners.py``), at ``seeds[b, cell]``."""
    roi = _check_args(pos, ids, age, epoch, flow_fw, flow_bw, roi, S)
    if seeds is not None:
        _check_seeds(seeds, ids.shape[0], ids.shape[1], flow_fw.device)
    if use_native(flow_fw):
        if seeds is not None:
            return tuple(ops().track_points_seeded(pos, ids, age, epoch, flow_fw, flow_bw, seeds, roi[0], roi[1],
                                                   roi[2], roi[3], int(S), float(alpha1), float(alpha2)))
        return tuple(ops().track_points(pos, ids, age, epoch, flow_fw, flow_bw, roi[0], roi[1], roi[2], roi[3],
                                        int(S), float(alpha1), float(alpha2)))
    return track_points_ref(pos, ids, age, epoch, flow_fw, flow_bw, roi, int(S), float(alpha1), float(alpha2), seeds)


class PointTracker:
    """The point grid of a stream of pairs, kept on the device.

    ``update(flow_fw, flow_bw=None, continuous=True)`` advances the state by one pair and returns
    ``track_points``'s outputs.  The first call seeds the grid, and so does any call with
    ``continuous`` false or after the batch, the frame shape, the device, the roi or the cell size
    changed: the points start at their seeds in the pair's first frame, with fresh ids, and take
    that pair's step.  Ids are never reused: ``epoch`` survives a reset (with another grid size it
    moves on to the first epoch whose ids lie above every id handed out so far; the bound is kept
    on the host, nothing is read back).

    ``seeds`` and ``first_seeds`` (B, N, 2) fp32, e.g. of ``ops.corners.corner_seeds``, replace the
    cells' centres: ``seeds`` serves the points born in this step, which live in the pair's second
    frame; ``first_seeds`` serves a (re)seeding of the grid, whose points start in the pair's first
    frame, and is not read by a pair that continues the last one."""

    def __init__(self, S: int = 32, roi: Optional[Sequence[int]] = None, alpha1: float = ALPHA1,
                 alpha2: float = ALPHA2):
        if int(S) < 1:
            raise ValueError(f"PointTracker: the cell size must be at least 1, got {S}")
        self.S = int(S)
        self.roi = None if roi is None else tuple(int(v) for v in roi)
        self.alpha1, self.alpha2 = float(alpha1), float(alpha2)
        self._state = None  # (pos, ids, age, epoch)
        self._sig = None
        self._next_id = 0  # host-side bound: every id handed out so far is below it
        self.resets = 0

    def reset(self) -> None:
        """Forget the points: the next update seeds the grid (with new ids)."""
        self._state = None

    def _seed(self, B: int, roi: Roi, device, seeds=None):
        pos, ids, age, epoch = seed_points(B, roi, self.S, device, seeds)
        N = ids.shape[1]
        # the ids handed out so far are below _next_id: start at the first epoch whose ids lie above
        e0 = -(-self._next_id // N)
        if e0 > 0:
            ids = ids + e0 * N
        self._next_id = (e0 + 1) * N
        epoch = epoch + e0
        self.resets += 1
        return pos, ids, age, epoch

    def update(self, flow_fw: torch.Tensor, flow_bw: Optional[torch.Tensor] = None, continuous: bool = True,
               roi: Optional[Sequence[int]] = None, seeds: Optional[torch.Tensor] = None,
               first_seeds: Optional[torch.Tensor] = None):
        if roi is not None:
            self.roi = tuple(int(v) for v in roi)
        B, _, H, W = flow_fw.shape
        use_roi = _check_grid((0, 0, W, H) if self.roi is None else self.roi, self.S)
        sig = (B, H, W, flow_fw.device, use_roi, self.S)
        seeded = self._state is None or not continuous or sig != self._sig
        if seeded:
            self._state = self._seed(B, use_roi, flow_fw.device, first_seeds)
            self._sig = sig
        pos, ids, age, epoch = self._state
        out = track_points(pos, ids, age, epoch, flow_fw, flow_bw, use_roi, self.S, self.alpha1, self.alpha2, seeds)
        pos_out, prev, ids_out, age_out, epoch_out, status, err2, counts = out
        self._state = (pos_out, ids_out, age_out, epoch_out)
        self._next_id += ids.shape[1]  # a step hands out ids below (epoch + 1) * N
        return out
