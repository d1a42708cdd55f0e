"""Inputs shared by the warm-start tests (tests/test_warm_start_{cpu,gpu}.py): small, non-square,
odd low-resolution flows with H * W no multiple of 64, each built for one way the forward splat
can go wrong.  Every case is a (B, 2, H, W) fp32 CPU tensor; oracles are computed once per case."""
import functools

import torch

SHAPES = [(16, 24), (17, 23)]
OUT = 1000.0  # a flow that leaves any of these images


def _randn(H, W, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    return sigma * torch.randn(2, H, W, generator=g)


def random_flow(H, W, sigma, seed):
    """Random flow, a 6 x 8 block of it shifted by (5.5, -3.25): its sources leave a hole."""
    f = _randn(H, W, sigma, seed)
    f[0, 4:10, 6:14] += 5.5
    f[1, 4:10, 6:14] -= 3.25
    return f


def random_batch(H, W, sigma):
    """(a): B = 2, different content per image."""
    return torch.stack([random_flow(H, W, sigma, 10 + int(sigma)), random_flow(H, W, sigma, 20 + int(sigma))])


def all_out(H, W):
    return torch.full((2, H, W), OUT)


def out_and_normal(H, W):
    """(b): one image without a valid point, one ordinary image."""
    return torch.stack([all_out(H, W), random_flow(H, W, 3.0, 5)])


def one_point(H, W):
    """(c): a single valid point; its flow fills the image (the search runs to the last ring)."""
    f = all_out(H, W)
    f[:, H - 1, W - 2] = torch.tensor([0.5, -0.25])
    g = all_out(H, W)
    g[:, 1, 1] = torch.tensor([-0.5, 0.25])
    return torch.stack([f, g])


# (d): two valid points at distance exactly 1 from a target; the one outside the R = 1 square of
# cells has the lower source index.  (source (x, y), flow) pairs, the target and its expected flow
RING_TIES = {
    "right": ([((2, 1), (4.0, 4.0)), ((10, 8), (-6.0, -3.0))], (5, 5), (4.0, 4.0)),   # (6, 5) vs (4, 5)
    "left": ([((2, 1), (2.0, 4.0)), ((10, 8), (-4.0, -3.0))], (5, 5), (2.0, 4.0)),    # (4, 5) vs (6, 5)
    "below": ([((2, 1), (3.0, 5.0)), ((10, 8), (-5.0, -4.0))], (5, 5), (3.0, 5.0)),   # (5, 6) vs (5, 4)
}


def ring_tie(H, W, name):
    f = all_out(H, W)
    for (x, y), (dx, dy) in RING_TIES[name][0]:
        f[0, y, x], f[1, y, x] = dx, dy
    return f[None]


def half_steps(H, W):
    """(e): flows from {-1.5, -0.5, 0.5, 1.5}^2 -- points on the half-integer lattice, many ties."""
    g = torch.Generator().manual_seed(7)
    return (torch.randint(0, 4, (1, 2, H, W), generator=g).float() - 1.5)


def constant(H, W):
    f = torch.empty(1, 2, H, W)
    f[:, 0], f[:, 1] = 0.25, -0.5
    return f


def zero_with_block(H, W):
    """Zero flow (row 0 and column 0 are invalid: x1 > 0 is strict) with a moved block."""
    f = torch.zeros(1, 2, H, W)
    f[0, 0, 3:7, 2:9], f[0, 1, 3:7, 2:9] = 6.0, 5.0
    return f


def collapse(H, W):
    """(f): flow = -0.95 (p - c): every point lands within 0.6 px of c, > 64 points in one cell."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cx, cy = W / 2 + 0.3, H / 2 + 0.4
    return torch.stack([-0.95 * (xs - cx), -0.95 * (ys - cy)])[None]


def non_finite(H, W):
    """(g): NaN and +-Inf at a few pixels of a random flow."""
    f = random_batch(H, W, 3.0)
    f[0, 0, 2, 3] = float("nan")
    f[0, 1, 5, 5] = float("nan")
    f[0, 0, 7, 1] = float("inf")
    f[1, 1, 9, 11] = float("-inf")
    f[1, :, 0, 0] = float("nan")
    return f


CASES = {
    "random3": lambda H, W: random_batch(H, W, 3.0),
    "random12": lambda H, W: random_batch(H, W, 12.0),
    "random40": lambda H, W: random_batch(H, W, 40.0),
    "all_out": lambda H, W: torch.stack([all_out(H, W)] * 2),
    "out_and_normal": out_and_normal,
    "one_point": one_point,
    "ring_right": lambda H, W: ring_tie(H, W, "right"),
    "ring_left": lambda H, W: ring_tie(H, W, "left"),
    "ring_below": lambda H, W: ring_tie(H, W, "below"),
    "half_steps": half_steps,
    "constant": constant,
    "zero_with_block": zero_with_block,
    "collapse": collapse,
    "non_finite": non_finite,
}
RANDOM = ("random3", "random12", "random40")


@functools.lru_cache(maxsize=None)
def case(name, shape):
    return CASES[name](*shape)


@functools.lru_cache(maxsize=None)
def oracle(name, shape):
    """(flow, gap) of forward_splat_nearest_ref on the case: computed once, never modified."""
    from raft_ros_amd.ops.reference import forward_splat_nearest_ref

    return forward_splat_nearest_ref(case(name, shape), return_gap=True)


@functools.lru_cache(maxsize=None)
def scipy_result(name, shape):
    from raft_ros_amd.utils.utils import forward_interpolate

    return torch.stack([forward_interpolate(x) for x in case(name, shape)])
