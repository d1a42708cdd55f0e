"""Shared cases of the corner-seed tests: frames, the parameter sets, a per-pixel loop oracle on
Python ints written independently of the vectorised reference, and synthetic patterns.

The specification is in integers, so no tolerance applies: every comparison is bitwise.
"""
import functools
import math
import os

import numpy as np
import torch

import track_cases as tc
from raft_ros_amd.ops.corners import corner_seeds_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 5), (5, 5), (37, 53), (64, 96)]
CELLS = [1, 4, 7, 8, 16, 200]  # 200: larger than every frame, a single cell
SCORE_MAX = 18727200


def same_pair(got, want, what=""):
    """(seeds, score) bitwise."""
    assert len(got) == len(want) == 2
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32, what
    assert tc.same(got[0], want[0]), f"{what}: seeds differ at {(got[0].cpu() != want[0].cpu()).nonzero()[:5].tolist()}"
    assert tc.same(got[1], want[1]), f"{what}: score differs at {(got[1].cpu() != want[1].cpu()).nonzero()[:5].tolist()}"


@functools.lru_cache(maxsize=None)
def frames(H, W, B=3):
    """(B, H, W, 3) uint8: noise over a smooth ramp, with a flat rectangle (score 0: centre
    fallback) and a saturated vertical edge (aperture) in the lower right; treat as read-only."""
    g = torch.Generator().manual_seed(97 * H + W)
    f = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    if H >= 8 and W >= 8:
        f[:, : H // 2, : W // 3] = 77
        f[:, H // 2:, 2 * W // 3:] = 0
        f[:, H // 2:, 2 * W // 3 + (W - 2 * W // 3) // 2:] = 255
    return f.contiguous()


def margins(S):
    """0, the default and the largest legal margin."""
    return sorted({0, S // 4, (S - 1) // 2})


# ---------------------------------------------------------------------------- the loop oracle
def loop_scores(frame):
    """The score of every pixel of one (H, W, 3) uint8 frame, in Python ints -> H lists of W ints.
    Asserts on the way that no intermediate leaves its range."""
    img = frame.tolist()
    H, W = len(img), len(img[0])
    g = [[(p[0] + 2 * p[1] + p[2] + 2) >> 2 for p in row] for row in img]

    def at(t, y, x):
        return t[min(max(y, 0), H - 1)][min(max(x, 0), W - 1)]

    ix = [[0] * W for _ in range(H)]
    iy = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            ix[y][x] = (at(g, y - 1, x + 1) + 2 * at(g, y, x + 1) + at(g, y + 1, x + 1)) - \
                       (at(g, y - 1, x - 1) + 2 * at(g, y, x - 1) + at(g, y + 1, x - 1))
            iy[y][x] = (at(g, y + 1, x - 1) + 2 * at(g, y + 1, x) + at(g, y + 1, x + 1)) - \
                       (at(g, y - 1, x - 1) + 2 * at(g, y - 1, x) + at(g, y - 1, x + 1))
            assert abs(ix[y][x]) <= 1020 and abs(iy[y][x]) <= 1020
    out = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            a = b = c = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    u, v = at(ix, y + dy, x + dx), at(iy, y + dy, x + dx)
                    a, b, c = a + u * u, b + u * v, c + v * v
            d = (a - c) * (a - c) + 4 * b * b
            assert 0 <= a <= 9363600 and 0 <= c <= 9363600 and d < 2 ** 53
            out[y][x] = (a + c) - math.isqrt(d)
            assert 0 <= out[y][x] <= SCORE_MAX
    return out


@functools.lru_cache(maxsize=None)
def loop_scores_of_case(H, W, b):
    return loop_scores(frames(H, W)[b])


def loop_seeds(scores, S, roi_size=None, origin=(0, 0), margin=None, min_score=0):
    """The seeds of one image from its per-pixel scores (lists), cell by cell -> (seeds (N, 2)
    fp32, score (N,) int32, the number of cells that fell back to their centre)."""
    H, W = len(scores), len(scores[0])
    w, h = (W, H) if roi_size is None else roi_size
    margin = S // 4 if margin is None else margin
    Gx, Gy = -(-w // S), -(-h // S)
    seeds, best, fallback = [], [], 0
    for gy in range(Gy):
        for gx in range(Gx):
            win = None  # (score, y, x): the first of the largest in index order
            for y in range(gy * S + margin, min(gy * S + S - margin, h)):
                for x in range(gx * S + margin, min(gx * S + S - margin, w)):
                    if win is None or scores[y][x] > win[0]:
                        win = (scores[y][x], y, x)
            if win is not None and win[0] > min_score:
                seeds.append((origin[0] + win[2], origin[1] + win[1]))
            else:
                seeds.append((origin[0] + min(gx * S + S // 2, w - 1), origin[1] + min(gy * S + S // 2, h - 1)))
                fallback += 1
            best.append(-1 if win is None else win[0])
    return torch.tensor(seeds, dtype=torch.float32), torch.tensor(best, dtype=torch.int32), fallback


def variants(H, W, S):
    """The parameter sets of one (shape, S): every margin, min_score 0 and the median winner score
    (about half the cells fall back), a non-zero origin and a roi smaller than the frame."""
    out = []
    for m in margins(S):
        base = corner_seeds_ref(frames(H, W)[:1], S, margin=m)[1]
        cand = base[base >= 0]
        med = int(cand.median()) if cand.numel() else 0
        out.append(dict(margin=m, min_score=0))
        out.append(dict(margin=m, min_score=med))
    out.append(dict(margin=None, min_score=0, origin=(3, 5)))
    if H > 2 and W > 3:
        out.append(dict(margin=None, min_score=0, origin=(1, 2), roi_size=(W - 3, H - 2)))
    return out


# ---------------------------------------------------------------------------- patterns
def gray_frame(g):
    """(H, W) integer levels -> (1, H, W, 3) uint8 with equal channels (gray = the level)."""
    return g.to(torch.uint8)[None, :, :, None].expand(1, *g.shape, 3).contiguous()


def checkerboard(H, W, period):
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return gray_frame(((y // period + x // period) % 2) * 255)


def stripes(H, W, period, vertical=True):
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return gray_frame((((x if vertical else y) // period) % 2) * 255)


def squares(H, W, S, lo=4, hi=11):
    """One bright square [lo, hi) x [lo, hi) in every S x S cell; its corner pixels are at lo and hi - 1."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    inside = (y % S >= lo) & (y % S < hi) & (x % S >= lo) & (x % S < hi)
    return gray_frame(inside * 200 + 20)


def demo_frame():
    from PIL import Image

    return torch.from_numpy(np.array(Image.open(os.path.join(ROOT, "demo-frames", "frame_0016.png")).convert("RGB")))[None]


@functools.lru_cache(maxsize=None)
def noise_frame(H=37, W=53):
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)


def fallback_share(frame, S, margin=0):
    """The share of cells the reference alone sends to their centre (score <= 0 or no candidate)."""
    score = corner_seeds_ref(frame, S, margin=margin)[1]
    return float((score <= 0).sum()) / score.numel()


# ---------------------------------------------------------------------------- a moving texture
@functools.lru_cache(maxsize=None)
def moving_texture(steps=tc.STEPS, H=37, W=53, B=2):
    """``steps + 1`` batches (B, H, W, 3) uint8 of a blocky texture shifted by a pixel a step."""
    g = torch.Generator().manual_seed(11)
    big = torch.randint(0, 256, (B, H // 3 + 4, W // 3 + 4, 3), generator=g, dtype=torch.uint8)
    big = big.repeat_interleave(3, dim=1).repeat_interleave(3, dim=2)
    return [big[:, k:k + H, k:k + W].contiguous() for k in range(steps + 1)]
