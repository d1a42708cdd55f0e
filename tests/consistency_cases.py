"""Seeded flow pairs, built on the host, shared by test_consistency_cpu.py / _gpu.py.

Non-zero magnitudes stay above 1e-6, so that no subnormal arises on either side of a comparison.
The expected results come from ``fb_consistency_ref`` on the host copy, computed once per field.
"""
import functools
import math

import numpy as np
import torch

from raft_ros_amd.ops.consistency import fb_consistency_ref

MIN_SHARE = 0.05  # every class covers at least this share of the parity field


def _no_tiny(t: torch.Tensor) -> torch.Tensor:
    tiny = (t != 0) & (t.abs() < 1e-6)
    return torch.where(tiny, torch.copysign(torch.full_like(t, 1e-6), t), t)


def gaussian(h, w, sigma, seed=0) -> torch.Tensor:
    return _no_tiny(torch.randn(2, h, w, generator=torch.Generator().manual_seed(seed)) * sigma)


def _smooth(x, y, H, W, amp):
    """An analytic forward flow with a drift to the right: a few pixels, gradients well below 1."""
    u = amp * (1.0 + 0.6 * torch.sin(2 * math.pi * y / H))
    v = amp * 0.4 * torch.cos(2 * math.pi * x / W)
    return u, v


def smooth_pair(H, W, amp=2.5, noise=0.1, patch=None, seed=0):
    """(fw, bw) of (2, H, W): fw smooth, bw = minus fw at the pixel that maps here (three fixed-point
    steps of the analytic field) plus noise, and ``patch = (y0, y1, x0, x1)`` of unrelated flow."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    fw = torch.stack(_smooth(x, y, H, W, amp))
    gu, gv = torch.zeros_like(x), torch.zeros_like(y)
    for _ in range(3):  # the source p of target q solves p = q - f(p)
        gu, gv = _smooth(x - gu, y - gv, H, W, amp)
    bw = -torch.stack([gu, gv]) + gaussian(H, W, noise, seed=seed)
    if patch is not None:
        y0, y1, x0, x1 = patch
        bw[:, y0:y1, x0:x1] = gaussian(y1 - y0, x1 - x0, 6.0, seed=seed + 1)
    return _no_tiny(fw).contiguous(), _no_tiny(bw).contiguous()


def class_shares(occ: torch.Tensor):
    return [(occ == k).double().mean().item() for k in range(3)]


@functools.lru_cache(maxsize=None)
def parity_pair():
    """37 x 41 (non-square, H * W odd) with every class on at least MIN_SHARE of the pixels."""
    fw, bw = smooth_pair(37, 41, patch=(8, 24, 10, 26), seed=3)
    shares = class_shares(fb_consistency_ref(fw[None], bw[None])[0])
    assert min(shares) >= MIN_SHARE, shares
    return fw, bw


def scaled_batch():
    """B = 3 of the parity field (odd H * W: unaligned image bases) at scales 1, 0.5 and 2."""
    fw, bw = parity_pair()
    return (torch.stack([fw, fw.flip(1) * 0.5, fw.flip(2) * 2.0]).contiguous(),
            torch.stack([bw, bw.flip(1) * 0.5, bw.flip(2) * 2.0]).contiguous())


def random_pair(h, w, seed=0):
    """Gaussian fw and bw; across a single row or column fw does not move, so that not every
    target leaves the frame."""
    fw, bw = gaussian(h, w, 1.5, seed=seed), gaussian(h, w, 1.5, seed=seed + 100)
    if h == 1:
        fw[1] = 0.0
    if w == 1:
        fw[0] = 0.0
    return fw, bw


# pixels of the edge field: (y, x) -> ((u, v), expected class or None where bw decides)
ULP_UP = float(np.nextafter(np.float32(1.0), np.float32(2.0)))  # 1 + 2^-23
EDGE_H, EDGE_W = 16, 24
EDGE_POINTS = {
    (3, 20): ((3.0, 0.0), None),            # target exactly at W-1: inside, the clamped neighbour weighs 0
    (10, 5): ((0.0, 5.0), None),            # target exactly at H-1
    (12, 19): ((4.0, 3.0), None),           # the corner (W-1, H-1)
    (4, 0): ((float(np.nextafter(np.float32(23.0), np.float32(24.0))), 0.0), 2),  # one ulp beyond W-1
    (0, 7): ((0.0, float(np.nextafter(np.float32(15.0), np.float32(16.0)))), 2),  # one ulp beyond H-1
    (6, 1): ((-ULP_UP, 0.0), 2),            # x + u = -2^-23: the first value below 0
    (1, 9): ((0.0, -ULP_UP), 2),            # y + v = -2^-23
    (8, 0): ((-0.0, 1.0), None),            # -0.0 at x = 0: inside
    (0, 11): ((1.0, -0.0), None),           # -0.0 at y = 0: inside
    (9, 23): ((0.0, 0.0), None),            # stays on the last column
    (15, 2): ((0.0, 0.0), None),            # stays on the last row
}


@functools.lru_cache(maxsize=None)
def edge_pair():
    """16 x 24, integer flow components (every target exactly integer) plus EDGE_POINTS; bw is
    finite everywhere, large on the last column and row (what a clamped neighbour reads)."""
    g = torch.Generator().manual_seed(11)
    fw = torch.randint(-3, 4, (2, EDGE_H, EDGE_W), generator=g).float()
    for (y, x), ((u, v), _) in EDGE_POINTS.items():
        fw[0, y, x], fw[1, y, x] = u, v
    bw = gaussian(EDGE_H, EDGE_W, 1.0, seed=12)
    bw[:, :, EDGE_W - 1] = 100.0 + torch.arange(EDGE_H, dtype=torch.float32)
    bw[:, EDGE_H - 1, :] = -200.0 - torch.arange(EDGE_W, dtype=torch.float32)
    return fw.contiguous(), bw.contiguous()


NONFINITE_FW = {(0, 2, 3): float("nan"), (1, 4, 5): float("inf"), (0, 6, 7): float("-inf"), (1, 8, 12): float("nan")}
NONFINITE_BW_NAN = (4, 9)     # bw[0] is NaN here ...
NONFINITE_SAMPLER = (3, 8)    # ... and this pixel's target (+0.5, +0.5) reads it with weight 1/4


@functools.lru_cache(maxsize=None)
def nonfinite_pair():
    """9 x 13: NaN and +-inf in fw (class 2), a NaN in bw at a sampled pixel (class 1, err2 NaN)."""
    fw, bw = gaussian(9, 13, 1.0, seed=4), gaussian(9, 13, 1.0, seed=5)
    for (c, y, x), val in NONFINITE_FW.items():
        fw[c, y, x] = val
    y, x = NONFINITE_SAMPLER
    fw[0, y, x], fw[1, y, x] = 0.5, 0.5
    bw[0][NONFINITE_BW_NAN] = float("nan")
    return fw.contiguous(), bw.contiguous()


@functools.lru_cache(maxsize=None)
def workload():
    """440 x 1024: ((fw, bw), the reference's (occ, err2, counts)), computed once."""
    fw, bw = smooth_pair(440, 1024, amp=6.0, noise=0.3, patch=(100, 300, 200, 700), seed=7)
    return (fw, bw), fb_consistency_ref(fw[None], bw[None])


def same(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bitwise equality as ``torch.equal`` sees it (shape, dtype, every value, infinities included),
    with a NaN equal to a NaN at the same place: ``torch.equal`` itself is false for any NaN, and
    which NaN an operation returns is not part of the arithmetic."""
    got, want = got.cpu(), want.cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not got.dtype.is_floating_point:
        return torch.equal(got, want)
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(got[~nan], want[~nan])


def check(got, want, what=""):
    """(occ, err2, counts) of the op against the reference's: all three bitwise."""
    names = ("occ", "err2", "counts")
    for name, g, w in zip(names, got, want):
        if not same(g, w):
            bad = int((g.cpu() != w.cpu()).sum()) if g.shape == w.shape else -1
            raise AssertionError(f"{what}: {name} differs from the reference ({bad} elements; shapes "
                                 f"{tuple(g.shape)} / {tuple(w.shape)}, dtypes {g.dtype} / {w.dtype})")


def loop_reference(fw: np.ndarray, bw: np.ndarray, alpha1: float, alpha2: float):
    """The specification pixel by pixel with numpy.float32 scalars, in its order: (2, H, W) arrays
    -> occ (H, W) uint8, err2 (H, W) float32, counts (2,)."""
    f32 = np.float32
    _, H, W = fw.shape
    occ, err2 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32)
    a1, a2 = f32(alpha1), f32(alpha2)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                u, v = f32(fw[0, y, x]), f32(fw[1, y, x])
                px, py = f32(x) + u, f32(y) + v
                if not (px >= 0 and px <= f32(W - 1) and py >= 0 and py <= f32(H - 1)):
                    occ[y, x], err2[y, x] = 2, np.inf
                    continue
                x0f, y0f = np.floor(px), np.floor(py)
                fx, fy = f32(px - x0f), f32(py - y0f)
                x0, y0 = int(x0f), int(y0f)
                x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
                s = []
                for c in (0, 1):
                    a00, a01, a10, a11 = (f32(bw[c, y0, x0]), f32(bw[c, y0, x1]), f32(bw[c, y1, x0]),
                                          f32(bw[c, y1, x1]))
                    top = f32(a00 + f32(fx * f32(a01 - a00)))
                    bot = f32(a10 + f32(fx * f32(a11 - a10)))
                    s.append(f32(top + f32(fy * f32(bot - top))))
                du, dv = f32(u + s[0]), f32(v + s[1])
                e = f32(f32(du * du) + f32(dv * dv))
                thr = f32(f32(a1 * f32(f32(f32(u * u) + f32(v * v)) + f32(f32(s[0] * s[0]) + f32(s[1] * s[1])))) + a2)
                occ[y, x], err2[y, x] = (0 if e <= thr else 1), e
    return occ, err2, np.array([(occ == 1).sum(), (occ == 2).sum()], np.int32)
